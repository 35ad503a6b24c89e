"""On-disk formats either side of the depth-map filter: PFM depth maps, ``*_cam.txt`` camera files,
``pair.txt`` view graphs and the per-scan folder layout ``test.py`` writes and its ``TTDataset`` reads back.

Host-side only (numpy); same function names, arguments and byte-level output as the reference:
``read_pfm`` / ``save_pfm`` (datasets/data_io.py:7-71), ``write_cam`` (test.py:149-167), ``read_camera_parameters``
(test.py:102-112), ``read_pair_file`` (test.py:136-146); ``load_filter_sample`` assembles what ``TTDataset.__getitem__``
(test.py:347-401) returns, minus the RGB image decode.  ``load_scene`` reads every view of a scan ONCE (with its image, through
PIL, imported on first use) for the scene-resident fusion; ``write_ply`` / ``read_ply`` are the binary PLY ``plyfile`` writes for
the reference's vertex array (test.py:461-471).
"""
from __future__ import annotations

import os
import re
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np


def read_pfm(filename) -> Tuple[np.ndarray, float]:
    """-> ``(data [H,W] or [H,W,3] float32, top row first; scale)``.  Raises on a bad magic or header."""
    with open(filename, "rb") as f:
        magic = f.readline().decode("utf-8").rstrip()
        if magic not in ("PF", "Pf"):
            raise Exception("Not a PFM file.")
        dims = re.match(r"^(\d+)\s(\d+)\s$", f.readline().decode("utf-8"))
        if not dims:
            raise Exception("Malformed PFM header.")
        width, height = int(dims.group(1)), int(dims.group(2))
        scale = float(f.readline().rstrip())
        order = "<" if scale < 0 else ">"                      # negative scale marks little-endian samples
        data = np.fromfile(f, order + "f")
    shape = (height, width, 3) if magic == "PF" else (height, width)
    return np.flipud(data.reshape(shape)), abs(scale)


def save_pfm(filename, image: np.ndarray, scale: float = 1) -> None:
    """Rows are stored bottom-up; greyscale ``[H,W]`` / ``[H,W,1]`` -> ``Pf``, ``[H,W,3]`` -> ``PF``; float32 only."""
    if image.dtype.name != "float32":
        raise Exception("Image dtype must be float32.")
    if image.ndim == 3 and image.shape[2] == 3:
        magic = "PF"
    elif image.ndim == 2 or (image.ndim == 3 and image.shape[2] == 1):
        magic = "Pf"
    else:
        raise Exception("Image must have H x W x 3, H x W x 1 or H x W dimensions.")
    little = image.dtype.byteorder == "<" or (image.dtype.byteorder == "=" and sys.byteorder == "little")
    with open(filename, "wb") as f:
        f.write(("%s\n%d %d\n%f\n" % (magic, image.shape[1], image.shape[0], -scale if little else scale)).encode("utf-8"))
        np.flipud(image).tofile(f)


def write_cam(file, cam) -> None:
    """``cam [2,4,4]``: extrinsic block, intrinsic 3x3 block, then the depth-range row ``cam[1][3]``."""
    rows = ["extrinsic"]
    rows += ["".join(str(cam[0][i][j]) + " " for j in range(4)) for i in range(4)]
    rows += ["", "intrinsic"]
    rows += ["".join(str(cam[1][i][j]) + " " for j in range(3)) for i in range(3)]
    rows += ["", " ".join(str(cam[1][3][j]) for j in range(4))]
    with open(file, "w") as f:
        f.write("\n".join(rows) + "\n")


def read_camera_parameters(filename) -> Tuple[np.ndarray, np.ndarray]:
    """-> ``(intrinsics [3,3], extrinsics [4,4])`` float32 from lines 1-4 and 7-9 of a ``*_cam.txt``."""
    with open(filename) as f:
        lines = [ln.rstrip() for ln in f.readlines()]
    extrinsics = np.array(" ".join(lines[1:5]).split(), dtype=np.float32).reshape(4, 4)
    intrinsics = np.array(" ".join(lines[7:10]).split(), dtype=np.float32).reshape(3, 3)
    return intrinsics, extrinsics


def read_pair_file(filename) -> List[Tuple[int, List[int]]]:
    """``pair.txt``: count, then per view its id and ``n id score id score ...``; views without sources are dropped."""
    out = []
    with open(filename) as f:
        for _ in range(int(f.readline())):
            ref = int(f.readline().rstrip())
            srcs = [int(x) for x in f.readline().rstrip().split()[1::2]]
            if srcs:
                out.append((ref, srcs))
    return out


def write_pair_file(filename, pairs, scores=None):
    """The inverse of ``read_pair_file``: ``pairs = [(view, [source, ...])]``, ``scores`` the matching list of score lists (None: every
    score is written as 0; the readers ignore it) -> ``filename``, so that ``read_pair_file(write_pair_file(path, x)) == x`` for every
    ``x`` whose views all have a source (``read_pair_file`` drops the others).  Returns ``filename``."""
    lines = [str(len(pairs))]
    for i, (ref, srcs) in enumerate(pairs):
        sc = [0.0] * len(srcs) if scores is None else list(scores[i])
        if len(sc) != len(srcs):
            raise ValueError("write_pair_file: view %d has %d sources and %d scores" % (ref, len(srcs), len(sc)))
        lines.append(str(int(ref)))
        lines.append(" ".join([str(len(srcs))] + ["%d %s" % (int(s), repr(float(c))) for s, c in zip(srcs, sc)]))
    with open(filename, "w") as f:
        f.write("\n".join(lines) + "\n")
    return filename


_COLMAP_PARAMS = {"SIMPLE_PINHOLE": 3, "PINHOLE": 4}         # f cx cy / fx fy cx cy


def _quat_to_rot(q) -> np.ndarray:
    """Unit quaternion (w, x, y, z) -> rotation matrix, float64 (normalised first)."""
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _rot_to_quat(R) -> np.ndarray:
    """Rotation matrix -> unit quaternion (w, x, y, z) with w >= 0 (the branch on the largest diagonal term)."""
    R = np.asarray(R, np.float64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = np.sqrt(tr + 1.0) * 2
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    else:
        i = int(np.argmax([R[0, 0], R[1, 1], R[2, 2]]))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
        q = [0.0, 0.0, 0.0, 0.0]
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    q = np.array(q)
    return q / np.linalg.norm(q) * (1.0 if q[0] >= 0 else -1.0)


def _data_lines(path) -> List[str]:
    with open(path) as f:
        return [ln.rstrip("\n") for ln in f if not ln.lstrip().startswith("#")]


def read_colmap_text(model_dir) -> Dict[str, object]:
    """A COLMAP sparse model exported as text (``cameras.txt``, ``images.txt``, ``points3D.txt``) -> the arrays of
    ``scene_prep.prepare_scene``.  The format is RECALLED, not read from a specification here:

    * ``cameras.txt``: ``CAMERA_ID MODEL WIDTH HEIGHT PARAMS...``; ``SIMPLE_PINHOLE`` (f cx cy) and ``PINHOLE`` (fx fy cx cy) only - any
      other model raises: like the original script, this needs undistorted input;
    * ``images.txt``: two lines per image, ``IMAGE_ID QW QX QY QZ TX TY TZ CAMERA_ID NAME`` (world to camera) and the 2-D points
      ``X Y POINT3D_ID ...`` (``-1``: no 3-D point);
    * ``points3D.txt``: ``POINT3D_ID X Y Z R G B ERROR`` and the track ``IMAGE_ID POINT2D_IDX ...``.  ``#`` lines are comments.

    Views are indexed in ascending ``IMAGE_ID``, points in ascending ``POINT3D_ID``; the observations are the track elements of
    ``points3D.txt`` (an image named twice in a track gives two observations; a track element whose image is not in ``images.txt``
    raises).  -> ``{"xyz" [N,3] float32, "obs_point" [M] int64, "obs_view" [M] int32, "R" [V,3,3] float32, "t" [V,3] float32,
    "K" [V,3,3] float32, "size" [V,2] int64 (width, height), "names", "image_ids" [V], "point_ids" [N]}``."""
    cams = {}
    for ln in _data_lines(os.path.join(model_dir, "cameras.txt")):
        tok = ln.split()
        if not tok:
            continue
        model = tok[1]
        if model not in _COLMAP_PARAMS:
            raise ValueError("read_colmap_text: camera %s has model %s; only PINHOLE and SIMPLE_PINHOLE (undistorted images) are supported"
                             % (tok[0], model))
        p = [float(x) for x in tok[4:]]
        if len(p) != _COLMAP_PARAMS[model]:
            raise ValueError("read_colmap_text: camera %s: %s takes %d parameters, got %d" % (tok[0], model, _COLMAP_PARAMS[model], len(p)))
        fx, fy, cx, cy = (p[0], p[0], p[1], p[2]) if model == "SIMPLE_PINHOLE" else p
        cams[int(tok[0])] = (np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64), int(tok[2]), int(tok[3]))
    images = {}
    lines = _data_lines(os.path.join(model_dir, "images.txt"))
    while lines and not lines[-1].strip():
        lines.pop()
    if len(lines) % 2:
        lines.append("")                                          # the last image has an empty line of 2-D points
    for head in lines[0::2]:
        tok = head.split()
        if len(tok) < 10:
            raise ValueError("read_colmap_text: images.txt: expected 'IMAGE_ID QW QX QY QZ TX TY TZ CAMERA_ID NAME', got %r" % head)
        cam_id = int(tok[8])
        if cam_id not in cams:
            raise ValueError("read_colmap_text: image %s uses camera %d, which cameras.txt does not hold" % (tok[0], cam_id))
        images[int(tok[0])] = ([float(x) for x in tok[1:5]], [float(x) for x in tok[5:8]], cam_id, " ".join(tok[9:]))
    if not images:
        raise ValueError("read_colmap_text: %s holds no image" % model_dir)
    image_ids = sorted(images)
    index = {iid: v for v, iid in enumerate(image_ids)}
    pts = {}
    for ln in _data_lines(os.path.join(model_dir, "points3D.txt")):
        tok = ln.split()
        if tok:
            pts[int(tok[0])] = ([float(x) for x in tok[1:4]], [int(x) for x in tok[8::2]])
    point_ids = sorted(pts)
    obs_point, obs_view = [], []
    for p, pid in enumerate(point_ids):
        for iid in pts[pid][1]:
            if iid not in index:
                raise ValueError("read_colmap_text: point %d is tracked in image %d, which images.txt does not hold" % (pid, iid))
            obs_point.append(p)
            obs_view.append(index[iid])
    return {"xyz": np.array([pts[pid][0] for pid in point_ids], np.float64).reshape(-1, 3).astype(np.float32),
            "obs_point": np.array(obs_point, np.int64), "obs_view": np.array(obs_view, np.int32),
            "R": np.stack([_quat_to_rot(images[i][0]) for i in image_ids]).astype(np.float32),
            "t": np.array([images[i][1] for i in image_ids], np.float64).astype(np.float32),
            "K": np.stack([cams[images[i][2]][0] for i in image_ids]).astype(np.float32),
            "size": np.array([cams[images[i][2]][1:] for i in image_ids], np.int64),
            "names": [images[i][3] for i in image_ids], "image_ids": np.array(image_ids, np.int64), "point_ids": np.array(point_ids, np.int64)}


def write_colmap_text(model_dir, xyz, obs_point, obs_view, R, t, K, size, names=None, model: str = "PINHOLE") -> None:
    """Writes the three text files ``read_colmap_text`` reads, one camera per image, ``IMAGE_ID`` = view + 1, ``POINT3D_ID`` = point + 1,
    numbers with ``repr`` (they read back exactly).  It exists so that tests can round-trip a synthetic model: images carry no 2-D points
    and tracks carry ``POINT2D_IDX`` 0.  ``model``: ``PINHOLE``, ``SIMPLE_PINHOLE`` (fx is written as f) or any other name, written with
    the PINHOLE parameters (for the test that such a model is refused)."""
    os.makedirs(model_dir, exist_ok=True)
    V = len(R)
    names = ["%08d.jpg" % v for v in range(V)] if names is None else list(names)
    num = lambda x: repr(float(x))  # noqa: E731
    with open(os.path.join(model_dir, "cameras.txt"), "w") as f:
        f.write("# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n")
        for v in range(V):
            k = np.asarray(K[v], np.float64)
            params = [k[0, 0], k[0, 2], k[1, 2]] if model == "SIMPLE_PINHOLE" else [k[0, 0], k[1, 1], k[0, 2], k[1, 2]]
            f.write("%d %s %d %d %s\n" % (v + 1, model, int(size[v][0]), int(size[v][1]), " ".join(num(x) for x in params)))
    with open(os.path.join(model_dir, "images.txt"), "w") as f:
        f.write("# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n"
                "#   POINTS2D[] as (X, Y, POINT3D_ID)\n")
        for v in range(V):
            q = _rot_to_quat(R[v])
            f.write("%d %s %s %d %s\n\n" % (v + 1, " ".join(num(x) for x in q), " ".join(num(x) for x in t[v]), v + 1, names[v]))
    tracks: Dict[int, List[int]] = {}
    for p, v in zip(np.asarray(obs_point).tolist(), np.asarray(obs_view).tolist()):
        tracks.setdefault(p, []).append(v)
    with open(os.path.join(model_dir, "points3D.txt"), "w") as f:
        f.write("# 3D point list with one line of data per point:\n#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n")
        for p in range(len(xyz)):
            track = " ".join("%d 0" % (v + 1) for v in tracks.get(p, []))
            f.write(("%d %s 128 128 128 0.0 %s" % (p + 1, " ".join(num(x) for x in xyz[p]), track)).rstrip() + "\n")


def _cam_2x4x4(path) -> np.ndarray:
    K, E = read_camera_parameters(path)
    cam = np.zeros((2, 4, 4), dtype=np.float32)
    cam[0] = E
    cam[1, :3, :3] = K
    cam[1, 3, 3] = 1.0
    return cam


def _confidence(scan_folder, vid) -> np.ndarray:
    path = os.path.join(scan_folder, "confidence/{:0>8}.npy".format(vid))
    if not os.path.exists(path):
        path = os.path.join(scan_folder, "confidence_v2/{:0>8}.npy".format(vid))
    return np.asarray(np.load(path), dtype=np.float32).transpose(2, 0, 1)          # [H,W,C] on disk -> [C,H,W]


def load_filter_sample(scan_folder, id_ref: int, id_srcs: Sequence[int], n_src_views: int = 10) -> Dict[str, np.ndarray]:
    """One ``TTDataset`` item (test.py:347-401) without the image: ``ref_depth [1,H,W]``, ``ref_cam [2,4,4]``,
    ``ref_conf [C,H,W]``, ``src_depths [V,1,H,W]``, ``src_cams [V,2,4,4]``, ``src_confs [V,C,H,W]``, ``ref_id``.
    Source views whose camera file is missing are skipped, as in the reference."""
    cam = lambda v: os.path.join(scan_folder, "cams/{:0>8}_cam.txt".format(v))  # noqa: E731
    depth = lambda v: np.array(read_pfm(os.path.join(scan_folder, "depth_est/{:0>8}.pfm".format(v)))[0], dtype=np.float32)  # noqa: E731
    srcs = [v for v in list(id_srcs)[:n_src_views] if os.path.exists(cam(v))]
    return {"ref_depth": depth(id_ref)[None], "ref_cam": _cam_2x4x4(cam(id_ref)), "ref_conf": _confidence(scan_folder, id_ref),
            "src_depths": np.stack([depth(v) for v in srcs])[:, None], "src_cams": np.stack([_cam_2x4x4(cam(v)) for v in srcs]),
            "src_confs": np.stack([_confidence(scan_folder, v) for v in srcs]), "ref_id": id_ref}


def save_depth_outputs(scan_folder, vid: int, depth: np.ndarray, confidences: np.ndarray, cam: np.ndarray) -> None:
    """What ``save_depth`` leaves per view for the filter to pick up (test.py:296-318): ``depth_est/%08d.pfm``,
    ``confidence/%08d.npy`` ([H,W,C]) and ``cams/%08d_cam.txt``."""
    for sub in ("depth_est", "confidence", "cams"):
        os.makedirs(os.path.join(scan_folder, sub), exist_ok=True)
    save_pfm(os.path.join(scan_folder, "depth_est/{:0>8}.pfm".format(vid)), np.ascontiguousarray(depth, dtype=np.float32))
    np.save(os.path.join(scan_folder, "confidence/{:0>8}.npy".format(vid)), np.asarray(confidences, dtype=np.float32))
    write_cam(os.path.join(scan_folder, "cams/{:0>8}_cam.txt".format(vid)), cam)


def read_img(path) -> np.ndarray:
    """-> uint8 ``[H,W,3]`` RGB.  (The reference's ``read_img`` returns this / 255. in float32; the point-cloud colours it writes are
    ``(that * 255).astype(uint8)``, which gives these bytes back for all 256 levels.)"""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def save_image(scan_folder, vid: int, img_uint8: np.ndarray) -> None:
    """``images/%08d.jpg`` of the per-scan folder (test.py:354 reads it back).  JPEG is lossy."""
    from PIL import Image
    os.makedirs(os.path.join(scan_folder, "images"), exist_ok=True)
    Image.fromarray(np.ascontiguousarray(img_uint8, dtype=np.uint8)).save(os.path.join(scan_folder, "images/{:0>8}.jpg".format(vid)))


def _image_path(scan_folder, vid) -> Optional[str]:
    for ext in ("jpg", "png"):
        path = os.path.join(scan_folder, "images/{:0>8}.{}".format(vid, ext))
        if os.path.exists(path):
            return path
    return None


def load_scene(pair_folder, scan_folder, n_src_views: int = 10) -> Dict[str, object]:
    """Every view that ``pair.txt`` uses, loaded ONCE: ``depths [Nv,H,W]``, ``confs [Nv,C,H,W]`` (a 2-D confidence file gives C = 1),
    ``cams [Nv,2,4,4]``, ``imgs [Nv,3,H,W]`` uint8 (``None`` without an ``images/`` folder), ``view_ids`` (the order of the stacks) and
    ``pairs``: ``[(ref_id, [src_id, ...])]`` in ``pair.txt`` order, sources truncated to ``n_src_views`` and those whose camera file is
    missing skipped (test.py:345, 369-371).  All views must share H x W (the reference stacks them)."""
    cam = lambda v: os.path.join(scan_folder, "cams/{:0>8}_cam.txt".format(v))  # noqa: E731
    pairs = []
    for id_ref, id_srcs in read_pair_file(os.path.join(pair_folder, "pair.txt")):
        srcs = [v for v in list(id_srcs)[:n_src_views] if os.path.exists(cam(v))]
        if not srcs:
            raise ValueError("view %d: none of its source views has a camera file" % id_ref)
        pairs.append((id_ref, srcs))
    view_ids: List[int] = []
    for id_ref, srcs in pairs:
        for v in [id_ref] + srcs:
            if v not in view_ids:
                view_ids.append(v)
    with_images = os.path.isdir(os.path.join(scan_folder, "images"))
    depths, confs, cams, imgs = [], [], [], []
    for v in view_ids:
        depths.append(np.array(read_pfm(os.path.join(scan_folder, "depth_est/{:0>8}.pfm".format(v)))[0], dtype=np.float32))
        path = os.path.join(scan_folder, "confidence/{:0>8}.npy".format(v))
        if not os.path.exists(path):
            path = os.path.join(scan_folder, "confidence_v2/{:0>8}.npy".format(v))
        c = np.asarray(np.load(path), dtype=np.float32)
        confs.append(c[None] if c.ndim == 2 else c.transpose(2, 0, 1))             # [H,W] or [H,W,C] on disk
        cams.append(_cam_2x4x4(cam(v)))
        if with_images:
            path = _image_path(scan_folder, v)
            if path is None:
                raise FileNotFoundError("no images/{:0>8}.jpg (or .png) in {}".format(v, scan_folder))
            imgs.append(read_img(path).transpose(2, 0, 1))
        shapes = {depths[0].shape, depths[-1].shape, confs[-1].shape[1:]} | ({imgs[-1].shape[1:]} if with_images else set())
        if len(shapes) != 1 or confs[-1].shape[0] != confs[0].shape[0]:
            raise ValueError("view %d: depth %s, confidence %s%s do not match the scene's %s" % (
                v, depths[-1].shape, confs[-1].shape, ", image %s" % (imgs[-1].shape,) if with_images else "", depths[0].shape))
    return {"depths": np.stack(depths), "confs": np.stack(confs), "cams": np.stack(cams),
            "imgs": np.ascontiguousarray(np.stack(imgs)) if with_images else None, "view_ids": view_ids, "pairs": pairs}


PLY_VERTEX_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
PLY_RECORD_BYTES = PLY_VERTEX_DTYPE.itemsize                   # 15


def ply_header(n: int) -> bytes:
    """What ``plyfile`` writes for ``PlyData([PlyElement.describe(vertex_all, 'vertex')])`` with ``PLY_VERTEX_DTYPE`` (test.py:461-471)."""
    lines = ["ply", "format binary_little_endian 1.0", "element vertex %d" % n, "property float x", "property float y", "property float z",
             "property uchar red", "property uchar green", "property uchar blue", "end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


def write_ply_records(path, records, n: int) -> None:
    """Header + ``n`` packed 15-byte vertex records (bytes, or a uint8 array / buffer of ``n * 15`` bytes)."""
    body = memoryview(np.ascontiguousarray(records)).cast("B") if not isinstance(records, (bytes, bytearray)) else records
    if len(body) != n * PLY_RECORD_BYTES:
        raise ValueError("write_ply_records: %d bytes for %d vertices of %d bytes" % (len(body), n, PLY_RECORD_BYTES))
    with open(path, "wb") as f:
        f.write(ply_header(n))
        f.write(body)


def write_ply(path, xyz: np.ndarray, rgb: np.ndarray) -> None:
    """``xyz [N,3]`` float32, ``rgb [N,3]`` uint8 -> binary little-endian PLY."""
    xyz, rgb = np.asarray(xyz), np.asarray(rgb)
    if xyz.ndim != 2 or xyz.shape[1] != 3 or rgb.shape != xyz.shape:
        raise ValueError("write_ply: xyz %s and rgb %s must both be [N,3]" % (xyz.shape, rgb.shape))
    if xyz.dtype != np.float32 or rgb.dtype != np.uint8:
        raise ValueError("write_ply: xyz must be float32 and rgb uint8, got %s and %s" % (xyz.dtype, rgb.dtype))
    v = np.empty(len(xyz), PLY_VERTEX_DTYPE)
    for i, k in enumerate(("x", "y", "z")):
        v[k] = xyz[:, i]
    for i, k in enumerate(("red", "green", "blue")):
        v[k] = rgb[:, i]
    write_ply_records(path, v.view(np.uint8), len(v))


def read_ply(path) -> Tuple[np.ndarray, np.ndarray]:
    """-> ``(xyz [N,3] float32, rgb [N,3] uint8)`` of a file in the layout ``write_ply`` writes; anything else is refused."""
    with open(path, "rb") as f:
        want = ply_header(0).split(b"\n")
        n = None
        for i, line in enumerate(want[:-1]):
            got = f.readline().rstrip(b"\r\n")
            if i == 2:
                m = re.match(rb"^element vertex (\d+)$", got)
                if not m:
                    raise ValueError("read_ply: expected 'element vertex N', got %r" % got)
                n = int(m.group(1))
            elif got != line:
                raise ValueError("read_ply: unsupported header line %r (expected %r)" % (got, line))
        v = np.fromfile(f, PLY_VERTEX_DTYPE)
    if len(v) != n:
        raise ValueError("read_ply: header says %d vertices, body holds %d" % (n, len(v)))
    xyz = np.stack([v["x"], v["y"], v["z"]], -1) if n else np.zeros((0, 3), np.float32)
    rgb = np.stack([v["red"], v["green"], v["blue"]], -1) if n else np.zeros((0, 3), np.uint8)
    return xyz.astype(np.float32, copy=False), rgb.astype(np.uint8, copy=False)


def read_alignment(path) -> np.ndarray:
    """The ``*_trans.txt`` of a Tanks-and-Temples training scene: 16 whitespace-separated numbers, a 4 x 4 matrix row by row whose last
    row is ``0 0 0 1`` -> float64 ``[4,4]``.  Anything else is refused."""
    with open(path) as f:
        tokens = f.read().split()
    try:
        values = [float(t) for t in tokens]
    except ValueError:
        raise ValueError("read_alignment: %s holds something that is not a number" % path)
    if len(values) != 16:
        raise ValueError("read_alignment: %s holds %d numbers, a 4x4 matrix has 16" % (path, len(values)))
    T = np.array(values, dtype=np.float64).reshape(4, 4)
    if not np.isfinite(T).all() or not np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError("read_alignment: %s: the matrix must be finite with the last row 0 0 0 1, got %s" % (path, T[3].tolist()))
    return T


def read_crop_volume(path) -> Dict[str, object]:
    """Open3D's ``SelectionPolygonVolume`` json (the ``<scene>.json`` of Tanks and Temples) -> ``{"orthogonal_axis": "X" | "Y" | "Z",
    "axis_min": float, "axis_max": float, "bounding_polygon": float64 [K,3]}``, what ``cloud_eval.crop_polygon`` / ``evaluate_tt`` take.
    Another ``class_name`` or a missing key is refused."""
    import json
    with open(path) as f:
        doc = json.load(f)
    if not isinstance(doc, dict) or doc.get("class_name") != "SelectionPolygonVolume":
        raise ValueError("read_crop_volume: %s: class_name must be 'SelectionPolygonVolume', got %r" % (
            path, doc.get("class_name") if isinstance(doc, dict) else type(doc).__name__))
    for key in ("orthogonal_axis", "axis_min", "axis_max", "bounding_polygon"):
        if key not in doc:
            raise ValueError("read_crop_volume: %s has no %r" % (path, key))
    axis = str(doc["orthogonal_axis"]).upper()
    if axis not in ("X", "Y", "Z"):
        raise ValueError("read_crop_volume: %s: orthogonal_axis must be X, Y or Z, got %r" % (path, doc["orthogonal_axis"]))
    poly = np.array(doc["bounding_polygon"], dtype=np.float64)
    if poly.ndim != 2 or poly.shape[1] != 3 or poly.shape[0] < 3 or not np.isfinite(poly).all():
        raise ValueError("read_crop_volume: %s: bounding_polygon must be K >= 3 finite xyz triples, got shape %s" % (path, poly.shape))
    return {"orthogonal_axis": axis, "axis_min": float(doc["axis_min"]), "axis_max": float(doc["axis_max"]), "bounding_polygon": poly}
