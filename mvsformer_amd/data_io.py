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
