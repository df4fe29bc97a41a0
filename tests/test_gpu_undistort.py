"""GPU: points, the new camera matrix, undistortion maps and remap (ccal_kernels_undistort.hip) against tests/undistort_ref.py,
an independent numpy f64 yardstick whose projection values come from oracle.project.

Bounds: pixel values of project / the round trip of unproject 1e-9 px (the suite's bound, tests/test_oracle_solver.py:122); unit
norm 1e-12; the new camera matrix 1e-12 relative to the formula on the device's own four unprojections; a map entry within half an
f32 ulp + 1e-9 of oracle.project; remap within 1 level of the f64 yardstick (the f32 sum errs by less than 65535 * 2^-22 levels:
the margin only covers near-ties of the rounding).  Inputs within 1e-12 relative of a validity boundary are left out, at most 0.1 %
(tests/test_undistort_cpu.py holds the inputs to that cap on the yardstick alone).

Known gap between the issue and the models: the 100-degree rotation has to show a non-empty NaN set "for every model", but KB4's
`project` is defined for every non-zero point (oracle/ccal_oracle.hpp:341), so its NaN set is empty by definition; the case
asserts that instead."""
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import undistort_ref as ref  # noqa: E402

from camera_intrinsic_calibration_rs_amd import _ffi, api, synth  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = ["ucm", "eucm", "kb4", "opencv5"]
W = H = 512
SIZES = [1, 63, 64, 65, 1000]
MAP_SIZES = [(37, 23), (130, 67), (512, 512)]
SW, SH = 64, 48                                  # remap source size


def _mp(name):
    m = synth.MODEL_NAMES[name]
    return m, np.asarray(synth.GT_PARAMS[m], dtype=np.float64)


def _roty(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])


# ---- 1. project -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("n", SIZES)
def test_project(gpu_ctx, oracle, name, n):
    m, p = _mp(name)
    xyz = ref.seeded_rays(m, n)
    uv, valid = gpu_ctx.project_points(m, p, xyz)
    v_ref, near = ref.project_valid(m, p, xyz)
    assert near.sum() <= 0.001 * n
    keep = ~near
    assert np.array_equal(valid[keep], v_ref[keep])
    assert np.isnan(uv[keep & ~v_ref]).all()
    ok = keep & v_ref
    if ok.any():
        d = np.abs(uv[ok] - oracle.project(m, p, xyz[ok])).max()
        print(f"project {name} n={n}: max |d| {d:.3e} px over {ok.sum()} valid rows")
        assert d <= 1e-9


# ---- 2. unproject ---------------------------------------------------------------------------------------------------------------
def _check_unproject(ctx, oracle, m, p, uv, p_oracle=None, small_radius=1e-8):
    rays, valid = ctx.unproject_points(m, p, uv)
    assert np.isnan(rays[~valid]).all() and np.isfinite(rays[valid]).all()
    if m in (ref.UCM, ref.EUCM):
        v_ref, near = ref.unproject_domain(m, p, uv)
        assert near.sum() <= 0.001 * len(uv)
        assert np.array_equal(valid[~near], v_ref[~near])
    assert valid.any()
    back = oracle.project(m, p if p_oracle is None else p_oracle, rays[valid])
    d = np.abs(back - uv[valid]).max()
    norm = np.linalg.norm(rays[valid], axis=1)
    small = np.zeros(valid.sum(), dtype=bool)
    if m == ref.KB4:
        small = np.hypot((uv[valid, 0] - p[2]) / p[0], (uv[valid, 1] - p[3]) / p[1]) < small_radius
        assert (rays[valid][small, 2] == 1.0).all()
    print(f"unproject model {m} n={len(uv)}: round trip {d:.3e} px, |norm - 1| {np.abs(norm[~small] - 1).max() if (~small).any() else 0:.3e}")
    assert d <= 1e-9
    assert (np.abs(norm[~small] - 1.0) <= 1e-12).all()
    return rays, valid


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("n", SIZES)
def test_unproject(gpu_ctx, oracle, name, n):
    m, p = _mp(name)
    rays, valid = _check_unproject(gpu_ctx, oracle, m, p, ref.seeded_pixels(p, n, W, H))
    if n == 1000 and m in (ref.UCM, ref.EUCM):
        assert (~valid).any()
    if n >= 63 and m == ref.KB4:
        assert rays[0].tolist() == [0.0, 0.0, 1.0]           # the principal point: below the small radius


@pytest.fixture()
def conventions(gpu_ctx):
    yield gpu_ctx.model_conventions()
    gpu_ctx.set_model_conventions(None)


def test_unproject_and_project_read_ocv5_order(gpu_ctx, oracle, conventions):
    m, p = _mp("opencv5")
    order = [2, 0, 4, 1, 3]                                    # k1 sits at slot 2, k2 at 0, p1 at 4, p2 at 1, k3 at 3
    for i, o in enumerate(order):
        conventions.ocv5_order[i] = o
    gpu_ctx.set_model_conventions(conventions)
    q = p.copy()
    for i, o in enumerate(order):
        q[4 + o] = p[4 + i]
    assert not np.array_equal(q, p)
    uv = ref.seeded_pixels(p, 65, W, H)
    _check_unproject(gpu_ctx, oracle, m, q, uv, p_oracle=p)
    xyz = ref.seeded_rays(m, 65)
    got, valid = gpu_ctx.project_points(m, q, xyz)
    assert np.abs(got[valid] - oracle.project(m, p, xyz[valid])).max() <= 1e-9
    K = ref.new_camera_matrix(ref.unproject_newton(oracle, m, p, ref.edge_midpoints(p, W, H)), 0.5, 37, 23)
    mp_ = gpu_ctx.undistort_map(m, q, K, (37, 23))
    xm, ym = mp_.download(); mp_.close()
    rx, ry, _ = ref.undistort_map(oracle, m, p, K, None, 37, 23)
    assert np.abs(xm - rx).max() < 1e-3 and np.abs(ym - ry).max() < 1e-3      # the order is read (values: test_maps)


def test_unproject_reads_the_small_radius(gpu_ctx, oracle, conventions):
    m, p = _mp("kb4")
    uv = np.array([[p[2] + 0.5, p[3] - 0.25], [p[2] + 30.0, p[3] + 40.0]])
    rays, valid = gpu_ctx.unproject_points(m, p, uv)
    assert valid.all() and abs(np.linalg.norm(rays[0]) - 1.0) <= 1e-12
    conventions.unproject_small_radius = 0.01                  # 0.5 px / 190.9 = 0.0029 is now below it
    gpu_ctx.set_model_conventions(conventions)
    rays2, valid2 = gpu_ctx.unproject_points(m, p, uv)
    assert valid2.all()
    assert rays2[0].tolist() == [0.5 / p[0], -0.25 / p[1], 1.0]
    assert np.array_equal(rays2[1], rays[1])


# ---- 3. the new camera matrix ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_new_camera_matrix(gpu_ctx, oracle, name):
    m, p = _mp(name)
    model = api.GenericModel(name, p, W, H)
    mid = ref.edge_midpoints(p, W, H)
    rays, valid = _check_unproject(gpu_ctx, oracle, m, p, mid)
    assert valid.all()
    for size in (None, (300, 200)):
        for balance in (0.0, 0.3, 1.0):
            K = model.estimate_new_camera_matrix_for_undistort(balance, size, ctx=gpu_ctx)
            Kr = ref.new_camera_matrix(rays, balance, *(size or (W, H)))
            assert K.shape == (3, 3) and np.allclose(K, Kr, rtol=1e-12, atol=0.0), (K, Kr)


def test_new_camera_matrix_none_when_a_midpoint_has_no_ray(gpu_ctx):
    p = list(synth.GT_PARAMS[synth.MODEL_EUCM])
    p[4] = 0.8                                                 # (W - 1, cy) leaves the domain: tests/test_undistort_cpu.py
    assert not ref.unproject_domain(ref.EUCM, p, ref.edge_midpoints(p, W, H))[0][1]
    assert api.GenericModel("eucm", p, W, H).estimate_new_camera_matrix_for_undistort(0.5, ctx=gpu_ctx) is None


# ---- 4. maps --------------------------------------------------------------------------------------------------------------------
_ROT = {"identity": None, "5deg": "rot5", "100deg_y": _roty(100.0)}


def _check_map(oracle, m, p, K, R, w, h, xm, ym, where):
    rx, ry, near = ref.undistort_map(oracle, m, p, K, R, w, h)
    assert xm.shape == (h, w) and xm.dtype == np.float32
    assert near.sum() <= 0.001 * w * h
    keep = ~near
    nan_ref = np.isnan(rx)
    assert np.array_equal(np.isnan(xm)[keep], nan_ref[keep]) and np.array_equal(np.isnan(ym)[keep], nan_ref[keep])
    ok = keep & ~nan_ref
    worst = 0.0
    for got, want in ((xm, rx), (ym, ry)):
        g, t = got[ok].astype(np.float64), want[ok]
        t32 = t.astype(np.float32)
        big = np.isinf(t32)                                    # beyond the f32 range: the correctly rounded map entry is that infinity
        assert np.array_equal(got[ok][big], t32[big])
        tol = 0.5 * np.spacing(np.abs(t32[~big])).astype(np.float64) + 1e-9
        err = np.abs(g[~big] - t[~big])
        if err.size:
            worst = max(worst, float((err / tol).max()))
        assert (err <= tol).all(), where
    print(f"map {where}: worst error {worst:.3f} of the bound, NaN {int(nan_ref.sum())} of {w * h}")
    return nan_ref


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("rot", list(_ROT))
def test_maps(gpu_ctx, oracle, name, rot):
    m, p = _mp(name)
    R = _ROT[rot]
    if isinstance(R, str):
        axis = np.array([0.5, -0.6, 0.3])
        R = synth.rodrigues(axis / np.linalg.norm(axis) * np.deg2rad(5.0))      # 5 degrees about a skew axis
    model = api.GenericModel(name, p, W, H)
    K_hand = np.array([[150.0, 0.0, 250.5], [0.0, 120.0, 260.25], [0.0, 0.0, 1.0]])      # fx != fy, for the 512 x 512 image
    for (w, h) in MAP_SIZES:
        K_est = model.estimate_new_camera_matrix_for_undistort(0.5, (w, h), ctx=gpu_ctx)
        for tag, K in (("K_est", K_est), ("K_hand", K_hand)):
            Ks = K.copy()
            if tag == "K_hand":
                Ks[0] *= w / float(W); Ks[1] *= h / float(H)     # the same field of view in the smaller image
            xm, ym = model.init_undistort_map(Ks, (w, h), rotation=R, ctx=gpu_ctx)
            nan_ref = _check_map(oracle, m, p, Ks, R, w, h, xm, ym, f"{name} {rot} {w}x{h} {tag}")
            if rot == "100deg_y":
                assert (~nan_ref).any()
                assert nan_ref.any() if name != "kb4" else not nan_ref.any()      # KB4 projects every non-zero point


# ---- 5. remap -------------------------------------------------------------------------------------------------------------------
def _images(dtype, ch, n, seed=3):
    rng = np.random.default_rng(seed)
    shape = (n, SH, SW) if ch == 1 else (n, SH, SW, ch)
    return rng.integers(0, np.iinfo(dtype).max + 1, shape, dtype=np.int64).astype(dtype)


def _random_maps(w, h, seed=5):
    rng = np.random.default_rng(seed + w)
    return (rng.uniform(-3.0, SW + 2.0, (h, w)).astype(np.float32), rng.uniform(-3.0, SH + 2.0, (h, w)).astype(np.float32))


def _edge_maps():
    xs = np.array([0.0, -0.0, SW - 1, 5.5, -1e-3, SW - 1 + 1e-3, np.nan, np.inf, -np.inf, 10.25, SW - 1.5], dtype=np.float32)
    ys = np.array([0.0, -0.0, SH - 1, 7.5, -1e-3, SH - 1 + 1e-3, np.nan, np.inf, -np.inf, SH - 1.25], dtype=np.float32)
    xm, ym = np.meshgrid(xs, ys)
    return np.ascontiguousarray(xm), np.ascontiguousarray(ym)


def _identity_maps():
    xm, ym = np.meshgrid(np.arange(SW, dtype=np.float32), np.arange(SH, dtype=np.float32))
    return np.ascontiguousarray(xm), np.ascontiguousarray(ym)


_MAPS = {"random37x23": lambda: _random_maps(37, 23), "random130x67": lambda: _random_maps(130, 67), "identity": _identity_maps,
         "edges": _edge_maps}
_PIX = [(np.uint8, 1), (np.uint8, 3), (np.uint16, 1)]


def _check_remap(out, imgs, xm, ym, where):
    exact = 0
    for i in range(len(imgs)):
        want, valid = ref.remap(imgs[i], xm, ym)
        diff = np.abs(out[i].astype(np.int64) - want.astype(np.int64))
        assert diff.max() <= 1, where
        assert (out[i][~valid] == 0).all()
        exact += int((diff == 0).sum())
    print(f"remap {where}: {exact / out.size:.6f} of the values equal the f64 yardstick exactly")
    return valid


@pytest.mark.parametrize("maps", list(_MAPS))
@pytest.mark.parametrize("dtype,ch", _PIX)
@pytest.mark.parametrize("n_img", [1, 3])
def test_remap(gpu_ctx, maps, dtype, ch, n_img):
    xm, ym = _MAPS[maps]()
    imgs = _images(dtype, ch, n_img)
    if n_img == 3:
        assert not np.array_equal(imgs[0], imgs[1]) and not np.array_equal(imgs[1], imgs[2])
    m = gpu_ctx.undistort_map_from_arrays(xm, ym)
    try:
        dx, dy = m.download()
        assert dx.tobytes() == xm.tobytes() and dy.tobytes() == ym.tobytes()
        out = m.remap(imgs)
    finally:
        m.close()
    assert out.dtype == imgs.dtype and out.shape == (n_img,) + xm.shape + imgs.shape[3:]
    valid = _check_remap(out, imgs, xm, ym, f"{maps} {np.dtype(dtype).name}x{ch} batch {n_img}")
    if maps == "identity":
        assert out.tobytes() == imgs.tobytes()
    if maps == "edges":
        want = np.ones(xm.shape, dtype=bool)
        want[:, [4, 5, 6, 7, 8]] = False; want[[4, 5, 6, 7, 8], :] = False
        assert np.array_equal(valid, want)
    if n_img == 1:
        assert np.array_equal(api.remap(imgs[0], xm, ym, ctx=gpu_ctx), out[0])


@pytest.mark.parametrize("dtype,ch", _PIX)
def test_remap_dev_equals_the_host_pointer_call(gpu_ctx, dtype, ch):
    import torch
    xm, ym = _random_maps(37, 23)
    imgs = _images(dtype, ch, 3)
    m = gpu_ctx.undistort_map_from_arrays(xm, ym)
    try:
        host = m.remap(imgs)
        raw = torch.from_numpy(imgs.view(np.uint8).reshape(-1).copy()).cuda()       # bytes: torch has no uint16 arithmetic to need
        dst = torch.full((host.nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        m.remap_dev(raw.data_ptr(), dst.data_ptr(), _ffi.PIX_U8 if dtype == np.uint8 else _ffi.PIX_U16, ch, SW, SH, 3)
        gpu_ctx.sync()
        assert dst.cpu().numpy().tobytes() == host.tobytes()
    finally:
        m.close()


@pytest.mark.parametrize("n_img", [1, 5])
@pytest.mark.parametrize("dtype,ch", _PIX)
def test_remap_dev_writes_every_byte_and_nothing_else(gpu_ctx, dtype, ch, n_img):
    """ccal_remap_dev writes into the caller's device memory: the destination lies in a torch block with 64 guard bytes on each side,
    every byte set to a fill beforehand.  With two fills, the guards keep theirs and every destination byte is the host-pointer
    call's - a byte the kernel skipped would keep one of the fills.  A 37 x 23 map: 851 pixels, no multiple of 4."""
    import torch
    xm, ym = _random_maps(37, 23)
    imgs = _images(dtype, ch, n_img)
    m = gpu_ctx.undistort_map_from_arrays(xm, ym)
    try:
        host = m.remap(imgs)
        raw = torch.from_numpy(imgs.view(np.uint8).reshape(-1).copy()).cuda()
        for fill in (0x5A, 0xA5):
            block = torch.full((host.nbytes + 128,), fill, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            m.remap_dev(raw.data_ptr(), block.data_ptr() + 64, _ffi.PIX_U8 if dtype == np.uint8 else _ffi.PIX_U16, ch, SW, SH, n_img)
            gpu_ctx.sync()
            got = block.cpu().numpy()
            assert (got[:64] == fill).all() and (got[-64:] == fill).all(), "bytes outside the destination were written"
            assert got[64:-64].tobytes() == host.tobytes(), fill
    finally:
        m.close()


def test_remap_refuses_bad_arguments(gpu_ctx):
    xm, ym = _identity_maps()
    m = gpu_ctx.undistort_map_from_arrays(xm, ym)
    try:
        buf = np.zeros((SH, SW, 3), dtype=np.uint16)
        import ctypes as C
        for dtype, ch, w, h, n in ((_ffi.PIX_U16, 3, SW, SH, 1), (_ffi.PIX_U8, 2, SW, SH, 1), (5, 1, SW, SH, 1), (_ffi.PIX_U8, 1, 0, SH, 1),
                                   (_ffi.PIX_U8, 1, SW, SH, 0)):
            rc = gpu_ctx.lib.ccal_remap(m.handle, dtype, ch, w, h, n, C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data))
            assert rc == _ffi.ERR_INVALID_ARG
        assert gpu_ctx.lib.ccal_remap(m.handle, _ffi.PIX_U8, 1, SW, SH, 1, None, C.c_void_p(buf.ctypes.data)) == _ffi.ERR_INVALID_ARG
    finally:
        m.close()
    h = C.c_void_p()
    p = np.asarray(synth.GT_PARAMS[synth.MODEL_KB4])
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    K = np.eye(3).reshape(9)
    assert gpu_ctx.lib.ccal_undistort_map_create(gpu_ctx.handle, 4, dp(p), dp(K), None, 8, 8, C.byref(h)) == _ffi.ERR_UNSUPPORTED
    assert gpu_ctx.lib.ccal_undistort_map_create(gpu_ctx.handle, 9, dp(p), dp(K), None, 8, 8, C.byref(h)) == _ffi.ERR_INVALID_ARG
    assert gpu_ctx.lib.ccal_undistort_map_create(gpu_ctx.handle, 2, dp(p), dp(K), None, 0, 8, C.byref(h)) == _ffi.ERR_INVALID_ARG
    assert gpu_ctx.lib.ccal_estimate_new_camera_matrix(gpu_ctx.handle, 2, dp(p), W, H, 1.5, 0, 0, dp(K)) == _ffi.ERR_INVALID_ARG


# ---- 6. end to end --------------------------------------------------------------------------------------------------------------
def _checkerboard():
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    return ((((xs // 16) + (ys // 16)) & 1) * 200 + (xs % 16) + 2 * (ys % 16)).astype(np.uint8)


@pytest.mark.parametrize("name", MODELS)
def test_end_to_end(gpu_ctx, oracle, name):
    m, p = _mp(name)
    model = api.GenericModel(name, p, W, H)
    img = _checkerboard()
    K = model.estimate_new_camera_matrix_for_undistort(0.5, ctx=gpu_ctx)
    xm, ym = model.init_undistort_map(K, (W, H), ctx=gpu_ctx)
    out = api.remap(img, xm, ym, ctx=gpu_ctx)
    # the yardstick, from the model parameters alone
    Kr = ref.new_camera_matrix(ref.unproject_newton(oracle, m, p, ref.edge_midpoints(p, W, H)), 0.5, W, H)
    rx, ry, near = ref.undistort_map(oracle, m, p, Kr, None, W, H)
    want, valid = ref.remap(img, rx, ry)
    with np.errstate(invalid="ignore"):
        edge = (np.abs(rx) < 1e-4) | (np.abs(rx - (W - 1)) < 1e-4) | (np.abs(ry) < 1e-4) | (np.abs(ry - (H - 1)) < 1e-4) | near
    assert edge.sum() <= 0.001 * W * H
    diff = np.abs(out.astype(np.int64) - want.astype(np.int64))[~edge]
    print(f"end to end {name}: {int((diff == 0).sum())} of {diff.size} pixels equal, {int(valid.sum())} inside the source")
    assert valid.sum() > 0.5 * W * H and diff.max() <= 1


# ---- 7. hygiene -----------------------------------------------------------------------------------------------------------------
def test_map_blocks_go_back_to_the_context(gpu_ctx):
    """A handle that is created, used and destroyed gives its blocks back to the context's cache (ccal_internal.hpp: ctx_alloc): 64
    cycles of a 2 MiB map and a 2 x 256 KiB remap do not lower the device's free memory (a leak would take 128 MiB + 32 MiB; the
    32 MiB allowance is for whatever else runs on the device meanwhile), and the second map equals the first bit for bit."""
    import torch
    m, p = _mp("eucm")
    model = api.GenericModel("eucm", p, W, H)
    K = model.estimate_new_camera_matrix_for_undistort(0.5, ctx=gpu_ctx)
    img = _checkerboard()[None]

    def cycle():
        h = gpu_ctx.undistort_map(m, p, K, (W, H))
        try:
            return h.download(), h.remap(img)
        finally:
            h.close()
    (x0, y0), o0 = cycle()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(64):
        (x1, y1), o1 = cycle()
    free1 = torch.cuda.mem_get_info()[0]
    assert x1.tobytes() == x0.tobytes() and y1.tobytes() == y0.tobytes() and o1.tobytes() == o0.tobytes()
    assert free0 - free1 < 32 << 20, (free0, free1)


# ---- on poisoned memory (the second library, CCAL_TEST_POISON_ALLOC=1; tests/test_gpu_poison.py describes the hook) ----------------
def _poison_case(ctx):
    from oracle import binding
    out = {}
    for name in MODELS:
        m, p = _mp(name)
        rays, valid = ctx.unproject_points(m, p, ref.edge_midpoints(p, W, H))
        K = ctx.estimate_new_camera_matrix(m, p, W, H, 0.5, (37, 23))
        h = ctx.undistort_map(m, p, K, (37, 23), _roty(100.0))
        out[f"{name}_x"], out[f"{name}_y"] = h.download()
        h.close()
        out[f"{name}_K"], out[f"{name}_rays"] = K, rays
    xm, ym = _random_maps(37, 23)
    h = ctx.undistort_map_from_arrays(xm, ym)
    for dtype, ch in _PIX:
        out[f"remap_{np.dtype(dtype).name}_{ch}"] = h.remap(_images(dtype, ch, 1))
    h.close()
    return out


def _poison_child(q, poison):
    sys.path.insert(0, ROOT)
    if poison:
        os.environ["CCAL_TEST_POISON_ALLOC"] = "1"
    from camera_intrinsic_calibration_rs_amd import _ffi as ffi
    assert ffi._lib is None
    ffi._lib = ffi.load_legacy()                                # the second library stands in for the product (test_gpu_poison.py)
    from camera_intrinsic_calibration_rs_amd.engine import Context
    ctx = Context(0, lib=ffi._lib)
    try:
        out = _poison_case(ctx)
    finally:
        ctx.close()
    q.put(out)


def _run_child(poison):
    cm = mp.get_context("spawn")
    q = cm.Queue()
    proc = cm.Process(target=_poison_child, args=(q, poison))
    proc.start()
    try:
        res = q.get(timeout=240)
    except Exception:
        if proc.is_alive():
            proc.kill()
        proc.join(10)
        raise AssertionError(f"the child process hung or crashed (exit code {proc.exitcode})")
    proc.join(60)
    assert proc.exitcode == 0
    return res


def test_maps_and_remap_on_poisoned_memory(oracle):
    clean, poisoned = _run_child(False), _run_child(True)
    assert clean.keys() == poisoned.keys()
    for k in clean:
        assert np.asarray(clean[k]).tobytes() == np.asarray(poisoned[k]).tobytes(), f"{k}: poisoned and clean runs differ"
    xm, ym = _random_maps(37, 23)
    for dtype, ch in _PIX:
        _check_remap(poisoned[f"remap_{np.dtype(dtype).name}_{ch}"], _images(dtype, ch, 1), xm, ym, f"poisoned {np.dtype(dtype).name}x{ch}")
    for name in MODELS:
        m, p = _mp(name)
        _check_map(oracle, m, p, poisoned[f"{name}_K"], _roty(100.0), 37, 23, poisoned[f"{name}_x"], poisoned[f"{name}_y"], f"poisoned {name}")
