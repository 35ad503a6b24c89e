"""Host side of the scan -> point cloud path (no GPU): the PLY the reference writes through ``plyfile`` (test.py:461-471), the
scene loader that reads every view of a scan once, and the 64-bit record offsets of the compaction."""
import os

import numpy as np
import pytest

VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])


def _header(n):
    return ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % n).encode("ascii")


@pytest.mark.parametrize("n", [0, 1, 1000])
def test_write_ply_bytes_and_round_trip(tmp_path, n):
    from mvsformer_amd import data_io
    rng = np.random.default_rng(n)
    xyz = (rng.standard_normal((n, 3)) * 500).astype(np.float32)
    rgb = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    if n:
        xyz[0, 1] = np.nan
        xyz[-1, 2] = -np.inf
    want = np.empty(n, VERTEX)
    for i, k in enumerate(("x", "y", "z")):
        want[k] = xyz[:, i]
    for i, k in enumerate(("red", "green", "blue")):
        want[k] = rgb[:, i]
    assert VERTEX.itemsize == 15
    path = str(tmp_path / "a.ply")
    data_io.write_ply(path, xyz, rgb)
    raw = open(path, "rb").read()
    assert raw[:len(_header(n))] == _header(n)
    assert len(raw) == len(_header(n)) + 15 * n and raw[len(_header(n)):] == want.tobytes()
    gx, gc = data_io.read_ply(path)
    assert gx.dtype == np.float32 and gx.shape == (n, 3) and gc.dtype == np.uint8 and gc.shape == (n, 3)
    assert np.array_equal(gx.view(np.uint32), xyz.view(np.uint32))            # bit-exact, NaN included
    assert np.array_equal(gc, rgb)
    # the record form (what the device writes) gives the same file
    path2 = str(tmp_path / "b.ply")
    data_io.write_ply_records(path2, np.frombuffer(want.tobytes(), np.uint8), n)
    assert open(path2, "rb").read() == raw
    with pytest.raises(ValueError):
        data_io.write_ply_records(path2, b"\0" * (15 * n + 1), n)
    with pytest.raises(ValueError):
        data_io.write_ply(path2, xyz.astype(np.float64), rgb)


def test_read_ply_refuses_other_layouts(tmp_path):
    from mvsformer_amd import data_io
    p = tmp_path / "c.ply"
    p.write_bytes(_header(1).replace(b"binary_little_endian", b"ascii") + b"\0" * 15)
    with pytest.raises(ValueError):
        data_io.read_ply(str(p))
    p.write_bytes(_header(2) + b"\0" * 15)                                       # header promises more than the body holds
    with pytest.raises(ValueError):
        data_io.read_ply(str(p))


def _write_scan(folder, n_views, h, w, pairs, skip_cam=(), sizes=None, images=False):
    from mvsformer_amd import data_io
    from PIL import Image
    rng = np.random.default_rng(5)
    cam = np.zeros((2, 4, 4), np.float32)
    cam[0] = np.eye(4)
    cam[1, :3, :3] = [[80, 0, w / 2], [0, 80, h / 2], [0, 0, 1]]
    cam[1, 3] = [425.0, 2.5, 192.0, 933.8]
    data = {}
    for v in range(n_views):
        hh, ww = (sizes or {}).get(v, (h, w))
        depth = (rng.random((hh, ww)) + 1).astype(np.float32)
        conf = rng.random((hh, ww, 3)).astype(np.float32)
        c = cam.copy()
        c[0, 0, 3] = float(v)
        data_io.save_depth_outputs(str(folder), v, depth, conf, c)
        img = rng.integers(0, 256, (hh, ww, 3)).astype(np.uint8)
        if images:
            os.makedirs(os.path.join(folder, "images"), exist_ok=True)
            Image.fromarray(img).save(os.path.join(folder, "images/%08d.png" % v))
        data[v] = (depth, conf, c, img)
    for v in skip_cam:
        os.remove(os.path.join(folder, "cams/%08d_cam.txt" % v))
    with open(os.path.join(folder, "pair.txt"), "w") as f:
        f.write("%d\n" % len(pairs))
        for ref, srcs in pairs:
            f.write("%d\n%d %s\n" % (ref, len(srcs), " ".join("%d 1.0" % s for s in srcs)))
    return data


def test_load_scene_reads_each_view_once(tmp_path, monkeypatch):
    from mvsformer_amd import data_io
    pairs = [(0, [1, 2, 3, 4]), (1, [0, 2, 5]), (2, [4, 3, 1, 0]), (3, []), (4, [2, 5, 0])]        # 5 has no camera file; 3 has no sources
    data = _write_scan(tmp_path, 6, 12, 20, pairs, skip_cam=(5,), images=True)
    calls = []
    real = data_io.read_pfm
    monkeypatch.setattr(data_io, "read_pfm", lambda p: (calls.append(os.path.basename(p)), real(p))[1])
    scene = data_io.load_scene(str(tmp_path), str(tmp_path), n_src_views=3)
    assert sorted(calls) == sorted(set(calls)) == ["%08d.pfm" % v for v in (0, 1, 2, 3, 4)]       # once each; 5 never
    want = [(r, [s for s in srcs[:3] if s != 5]) for r, srcs in data_io.read_pair_file(str(tmp_path / "pair.txt"))]
    assert [r for r, _ in want] == [0, 1, 2, 4]                                                  # view 3 has no sources: no job
    assert scene["pairs"] == want
    ids = scene["view_ids"]
    assert sorted(ids) == [0, 1, 2, 3, 4] and len(ids) == 5
    assert scene["depths"].shape == (5, 12, 20) and scene["confs"].shape == (5, 3, 12, 20) and scene["cams"].shape == (5, 2, 4, 4)
    assert scene["imgs"].shape == (5, 3, 12, 20) and scene["imgs"].dtype == np.uint8
    for i, v in enumerate(ids):
        depth, conf, cam, img = data[v]
        assert np.array_equal(scene["depths"][i], depth) and np.array_equal(scene["confs"][i], conf.transpose(2, 0, 1))
        assert np.array_equal(scene["cams"][i][0], cam[0]) and np.array_equal(scene["cams"][i][1, :3, :3], cam[1, :3, :3])
        assert np.array_equal(scene["imgs"][i], img.transpose(2, 0, 1))                          # PNG: exact
    assert np.array_equal(data_io.read_img(str(tmp_path / "images/00000002.png")), data[2][3])


def test_load_scene_without_images_and_with_mismatched_sizes(tmp_path):
    from mvsformer_amd import data_io
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    _write_scan(a, 3, 8, 10, [(0, [1, 2]), (1, [0, 2])])
    assert data_io.load_scene(str(a), str(a))["imgs"] is None
    _write_scan(b, 3, 8, 10, [(0, [1, 2]), (1, [0, 2])], sizes={2: (8, 12)})
    with pytest.raises(ValueError):
        data_io.load_scene(str(b), str(b))


def test_save_image_layout(tmp_path):
    from mvsformer_amd import data_io
    img = np.full((16, 24, 3), 128, np.uint8)
    data_io.save_image(str(tmp_path), 7, img)
    got = data_io.read_img(str(tmp_path / "images/00000007.jpg"))
    assert got.shape == (16, 24, 3) and got.dtype == np.uint8 and np.abs(got.astype(int) - 128).max() <= 2    # JPEG is lossy


def test_record_offsets_are_64_bit():
    """A cloud's byte offsets pass 2^31 from 143 M points on (49 full views of 1536x1152 stay below: 1.3e9 bytes; 200 do not): the byte
    offset of a record and the workspace size come back as int64."""
    from mvsformer_amd import _lib
    lib = _lib.load()
    n = 200 * 1536 * 1152
    assert 15 * n > 2 ** 31
    assert lib.mvs_pointcloud_record_offset(n) == 15 * n
    assert lib.mvs_pointcloud_record_offset(2 ** 40 + 3) == 15 * (2 ** 40 + 3)
    blocks = 49 * ((1536 * 1152 + 255) // 256)
    assert lib.mvs_pointcloud_workspace_bytes(49, 1152, 1536) == (blocks + 1) * 8 + blocks * 4
    assert lib.mvs_pointcloud_workspace_bytes(0, 4, 4) < 0 and lib.mvs_geo_filter_scene_workspace_bytes(3, 0) < 0
    assert lib.mvs_geo_filter_scene_workspace_bytes(49, 10) == 49 * lib.mvs_geo_filter_workspace_bytes(1, 10)
    # bad calls are refused before any launch
    assert lib.mvs_pointcloud_scatter(None, None, None, 1, 1, 4, 4, None, None, 0, None, 1, None, None, None, None) < 0
    assert b"mvs_pointcloud_scatter" in lib.mvs_last_error()
    assert lib.mvs_geo_filter_dynamic_scene_fwd(None, None, None, 1, None, None, None, 1, 2, 4, 4, 4.0, 1300.0, None, None, None, None, None) < 0


def test_scene_fusion_refuses_cpu_tensors_and_bad_arguments():
    import torch
    from mvsformer_amd import fusion
    from mvsformer_amd._lib import MvsHipError
    sc = fusion.SceneFusion("pcd", [0.5])
    with pytest.raises(MvsHipError):
        sc.add_view(0, torch.ones(4, 4), torch.ones(1, 4, 4), torch.zeros(2, 4, 4))
    with pytest.raises(ValueError):
        fusion.SceneFusion("gipuma", [0.5])
    with pytest.raises(ValueError):
        sc.fuse()
