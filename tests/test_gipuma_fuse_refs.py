"""Host side of the gipuma-style fusion (no GPU): the numpy restatement of the rule against a plain per-pixel loop, the fp64 tables against
the oracle's projection chain, and the argument checks of ``mvs_gipuma_fuse_scene`` (refused before anything is enqueued)."""
import numpy as np
import pytest
import torch

import gipuma_fuse_util as gu


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _rounded_once(a32, a64):
    """``a32`` is ``a64`` rounded to float32 (2^-24 relative), give or take the last float64 bits of a differently ordered product."""
    return bool(np.all(np.abs(a32.astype(np.float64) - a64) <= 2.0 ** -23 * np.abs(a64) + 1e-13 * np.abs(a64).max()))


def test_vectorised_rule_equals_the_pixel_loop():
    from mvsformer_amd import fusion
    depths, _, cams, _ = gu.make_scene(5, 9, 11, seed=1)
    tables = fusion.gipuma_tables(cams)
    jobs_list = [None, [(3, [0, 4]), (0, [4, 3, 2, 1]), (1, [2])]]
    for jobs in jobs_list:
        for kw in (dict(), dict(disp_thresh=1.0, num_consistent=1)):
            a, b = gu.gipuma_rule(depths, tables, jobs, **kw), gu.gipuma_rule_pixelwise(depths, tables, jobs, **kw)
            for k in ("keep", "used", "count", "points"):
                assert np.array_equal(_bits(a[k]), _bits(b[k])), (jobs, kw, k)
    a = gu.gipuma_rule(depths, tables)
    assert a["keep"][0].mean() > 0.5 and a["used"].any() and a["keep"][1:].sum() < a["keep"][0].sum()
    # consistent pairs of kept pixels are exactly what `used` records
    assert int(a["used"].sum()) <= int((a["consistent"] & a["keep"][:, None]).sum())


def test_tables_agree_with_the_oracle_projection_chain():
    """``A, b`` against ``oracle.ref_fusion``'s chain img_to_cam -> cam_to_world -> world_to_cam -> cam_to_img (what ``project_img`` runs) and
    ``B, c`` against its first half, in float64 at integer pixel coordinates, to 1e-9 relative.  The chain adds 1e-9 to every homogeneous
    divisor.  Three of the four additions scale all homogeneous coordinates alike and drop out when the result is divided by its own w
    (or by its z, for a pixel position; there 1e-9 stands beside z ~ 600).  The first one, in ``img_to_cam``, divides a ray with z = 1 by
    (1 + 1e-9) before the depth is applied, i.e. it shortens the depth by that factor: the chain is given depth * (1 + 1e-9), so that
    the bound measures the tables and not the oracle's epsilon."""
    from mvsformer_amd import fusion
    from oracle import ref_fusion as rf
    nv, h, w = 4, 6, 7
    depths, _, cams, _ = gu.make_scene(nv, h, w, seed=7)
    # the rule takes the camera centre as -R^T t, the chain inverts the 4x4 matrix: the two agree as far as R is orthogonal, so the
    # float32 rotations of the scene (orthogonal to 6e-8) are made orthogonal to float64 precision first
    cams = cams.astype(np.float64)
    for v in range(nv):
        U, _, Vt = np.linalg.svd(cams[v, 0, :3, :3])
        cams[v, 0, :3, :3] = U @ Vt
    cams64 = torch.from_numpy(cams)
    R, t, K = cams64[:, 0, :3, :3].numpy(), cams64[:, 0, :3, 3].numpy(), cams64[:, 1, :3, :3].numpy()
    B32, c32, A32, b32, fb32 = fusion.gipuma_tables(cams)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    grid = torch.from_numpy(np.stack([xs, ys, np.ones_like(xs)], -1))[None, ..., None]        # [1,h,w,3,1] integer pixels
    worst = 0.0
    for r in range(nv):
        d = torch.from_numpy(depths[r]).double()[None, None] * (1.0 + 1e-9)
        cam_r = cams64[r][None]
        wld = rf.cam_to_world(rf.img_to_cam(grid, d, cam_r), cam_r)                            # [1,h,w,4,1]
        Xc = (wld[..., :3, 0] / wld[..., 3:4, 0]).numpy()[0]
        X = (B32[r].astype(np.float64) @ np.stack([xs, ys, np.ones_like(xs)], 0).reshape(3, -1)).reshape(3, h, w) * depths[r] \
            + c32[r].astype(np.float64)[:, None, None]
        # float32 rounding of a table entry is 2^-24 relative: compare the fp64 tables themselves (recomputed), then the rounding
        B64 = R[r].T @ np.linalg.inv(K[r])
        c64 = -R[r].T @ t[r]
        X64 = (B64 @ np.stack([xs, ys, np.ones_like(xs)], 0).reshape(3, -1)).reshape(3, h, w) * depths[r] + c64[:, None, None]
        scale = np.abs(Xc).max()
        worst = max(worst, np.abs(X64.transpose(1, 2, 0) - Xc).max() / scale)
        assert np.abs(X - X64).max() / scale < 4 * 2.0 ** -24
        assert _rounded_once(B32[r], B64) and _rounded_once(c32[r], c64)
        for s in range(nv):
            if s == r:
                continue
            cam_s = cams64[s][None]
            cs = rf.world_to_cam(wld, cam_s)
            q = rf.cam_to_img(cs, cam_s)[0, ..., :2, 0].numpy()                                # [h,w,2]
            zc = (cs[..., 2, 0] / cs[..., 3, 0]).numpy()[0]
            P = K[s] @ np.concatenate([R[s], t[s][:, None]], 1)
            A64, b64 = P[:, :3] @ B64, P[:, :3] @ c64 + P[:, 3]
            fb64 = K[r][0, 0] * np.linalg.norm(c64 - (-R[s].T @ t[s]))
            assert _rounded_once(A32[r, s], A64) and _rounded_once(b32[r, s], b64)
            assert _rounded_once(fb32[r, s:s + 1], np.array([fb64]))
            qq = (A64 @ np.stack([xs, ys, np.ones_like(xs)], 0).reshape(3, -1)).reshape(3, h, w) * depths[r] + b64[:, None, None]
            u, v, z = qq[0] / qq[2], qq[1] / qq[2], qq[2]
            worst = max(worst, np.abs(u - q[..., 0]).max() / max(w, np.abs(q[..., 0]).max()),
                        np.abs(v - q[..., 1]).max() / max(h, np.abs(q[..., 1]).max()), (np.abs(z - zc) / np.abs(zc)).max())
    print("worst relative difference to the chain: %.3e" % worst)
    assert worst < 1e-9


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    from mvsformer_amd import _lib
    lib = _lib.load()
    assert "mvs_gipuma_fuse_scene" in _lib.SIGNATURES and len(_lib.SIGNATURES["mvs_gipuma_fuse_scene"][1]) == 23
    assert lib.mvs_version() == _lib.ABI_VERSION                # an addition: the version the older tests pin (51) stands
    p = 0x1000                                                  # never dereferenced: every call below is refused on the host

    def call(depth=p, B=p, c=p, A=p, b=p, fb=p, nv=3, ref=None, src=None, ns=None, R=3, V=2, h=4, w=4, th=(0.2, 3.0, 0.001, 1e5),
             used=p, keep=p, count=None, points=p):
        return lib.mvs_gipuma_fuse_scene(depth, B, c, A, b, fb, nv, ref, src, ns, R, V, h, w, *th, used, keep, count, points, None)

    for name in ("depth", "B", "c", "A", "b", "fb", "used", "keep", "points"):
        assert call(**{name: None}) < 0, name
        assert b"mvs_gipuma_fuse_scene" in lib.mvs_last_error()
    assert call(nv=1, R=1, V=0) < 0                             # one view has no sources
    assert call(h=0) < 0 and call(w=0) < 0 and call(h=-4) < 0 and call(w=2 ** 24 + 1) < 0
    assert call(R=2) < 0 and call(V=3) < 0                      # without a table R = Nv and Vmax = Nv - 1
    assert call(ref=p) < 0 and call(ref=p, src=p) < 0 and call(src=p, ns=p) < 0          # a table given in part
    assert call(ref=p, src=p, ns=p, R=0) < 0 and call(ref=p, src=p, ns=p, V=0) < 0 and call(ref=p, src=p, ns=p, V=3) < 0
    assert call(ref=p, src=p, ns=p, R=65536) < 0
    assert call(th=(float("nan"), 3.0, 0.001, 1e5)) < 0 and call(th=(0.2, float("nan"), 0.001, 1e5)) < 0


def test_python_layer_refuses_cpu_tensors_and_bad_jobs():
    from mvsformer_amd import fusion, ops
    from mvsformer_amd._lib import MvsHipError
    with pytest.raises(ValueError):
        fusion.SceneFusion("gipuma", [0.5])                     # the third route is a class of its own, not a `method`
    sc = fusion.GipumaFusion([0.5])
    assert sc.method == "gipuma" and (sc.disp_threshold, sc.num_consistent, sc.depth_min, sc.depth_max) == (0.2, 3, 0.001, 100000.0)
    with pytest.raises(MvsHipError):
        sc.add_view(0, torch.ones(4, 4), torch.ones(1, 4, 4), torch.zeros(2, 4, 4))
    with pytest.raises(ValueError):
        sc.fuse()
    with pytest.raises(ValueError):
        fusion.GipumaFusion([0.5], depth_min=-1.0)
    with pytest.raises(ValueError):
        fusion.gipuma_tables(np.zeros((3, 4, 4)))
    tabs = tuple(torch.from_numpy(t) for t in fusion.gipuma_tables(gu.make_scene(3, 4, 4, 0)[2]))
    with pytest.raises(MvsHipError):
        ops.gipuma_fuse_scene(torch.ones(3, 4, 4), tabs)
    assert [t.shape for t in tabs] == [(3, 3, 3), (3, 3), (3, 3, 3, 3), (3, 3, 3), (3, 3)] and all(t.dtype == torch.float32 for t in tabs)
