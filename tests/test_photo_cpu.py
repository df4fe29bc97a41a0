"""CPU: the photometric stage's host side (ccal_photo_set_defaults, ccal_photo_tables, the argument checks that precede any use of the
device) and tests/photo_ref.py, its numpy yardstick, on its own.  The device is held to the yardstick in tests/test_gpu_photo.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import photo_ref as pr  # noqa: E402

from camera_intrinsic_calibration_rs_amd import _ffi, api, engine  # noqa: E402


def _ulps(a, b):
    """The distance of two arrays of finite non-negative doubles in units in the last place."""
    return np.abs(np.asarray(a, dtype=np.float64).view(np.int64) - np.asarray(b, dtype=np.float64).view(np.int64))


SIGMAS = [0.0, 1e-300, 0.1, 1.0 / 3.0, 0.34, 0.5, 1.0, 1.2, 2.0, 3.0, 4.999, 5.0, 5.3, 16.0 / 3.0]


@pytest.mark.parametrize("sigma", SIGMAS)
def test_tables_against_numpy(sigma):
    """The radius exactly; taps and T within 4 ulp (libm is not pinned); the taps of the whole kernel sum to 1 within 1e-15."""
    o = pr.opts(blur_sigma=sigma, noise_read=1.7, noise_shot=0.043)
    r, taps, T = engine.photo_tables(api.PhotoOpts(**o))
    r_ref, taps_ref, T_ref = pr.tables(o)
    assert r == r_ref == min(16, int(np.ceil(3.0 * sigma)))
    assert taps.shape == (17,) and T.shape == (256,)
    assert (taps[r + 1:] == 0.0).all() and (taps[:r + 1] >= 0.0).all() and taps[0] > 0.0
    assert _ulps(taps, taps_ref).max() <= 4, (sigma, _ulps(taps, taps_ref).max())
    assert _ulps(T, T_ref).max() <= 4
    assert abs((taps[0] + 2.0 * taps[1:].sum()) - 1.0) < 1e-15
    assert (np.diff(taps[:r + 1]) <= 0.0).all()


def test_sigma_zero_is_one_tap_of_one_and_no_noise_is_a_table_of_zeros():
    r, taps, T = engine.photo_tables(api.PhotoOpts())
    assert r == 0 and taps[0] == 1.0 and not taps[1:].any() and not T.any()
    r, taps, T = engine.photo_tables(api.PhotoOpts(noise_read=2.0))
    assert (T == 2.0).all()
    r, taps, T = engine.photo_tables(api.PhotoOpts(noise_shot=0.25))
    assert T[0] == 0.0 and T[4] == 1.0 and T[100] == 5.0


def test_defaults_are_off():
    o = _ffi.PhotoOpts(1.0, 2.0, 3.0, 4.0, 5.0, 6, 7)
    assert _ffi.load().ccal_photo_set_defaults(C.byref(o)) == _ffi.OK
    assert [getattr(o, f) for f, _ in _ffi.PhotoOpts._fields_] == [0.0, 0.0, 1.0, 0.0, 0.0, 0, 0]
    assert _ffi.load().ccal_photo_set_defaults(None) == _ffi.ERR_INVALID_ARG
    d = api.PhotoOpts()
    assert [getattr(d, f) for f, _ in _ffi.PhotoOpts._fields_] == [0.0, 0.0, 1.0, 0.0, 0.0, 0, 0]
    assert [f for f, _ in _ffi.PhotoOpts._fields_] == list(pr.OFF)
    assert C.sizeof(_ffi.PhotoOpts) == 56


def test_the_header_states_the_struct_the_binding_has():
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "ccal.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} ccal_photo_opts;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(?:double|uint64_t|int64_t)\s+([a-z_0-9]+)\s*;", body)
    assert fields == [f for f, _ in _ffi.PhotoOpts._fields_]
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    rust = re.search(r"pub struct ccal_photo_opts \{(.*?)\n\}", doc, flags=re.S).group(1)
    assert re.findall(r"pub ([a-z_0-9]+):", rust) == fields


# ---- the yardstick alone ----------------------------------------------------------------------------------------------------------------
def _random(dtype, n=2, h=23, w=31, seed=5):
    return np.random.default_rng(seed).integers(0, np.iinfo(dtype).max + 1, (n, h, w)).astype(dtype)


def test_yardstick_identity_with_all_effects_off():
    o = pr.opts()
    for dtype in (np.uint8, np.uint16):
        src = _random(dtype)
        assert np.array_equal(pr.apply(src, dtype, pr.tables(o), o), src)
    every = np.arange(65536, dtype=np.uint16).reshape(1, 256, 256)
    assert np.array_equal(pr.apply(every, np.uint16, pr.tables(o), o), every)
    assert np.array_equal(pr.apply(every, np.uint8, pr.tables(o), o), np.rint(every / 257.0).astype(np.uint8))
    levels = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)
    assert np.array_equal(pr.apply(levels, np.uint16, pr.tables(o), o), levels.astype(np.uint16) * 257)


@pytest.mark.parametrize("sigma", [0.4, 1.2, 16.0 / 3.0])
def test_yardstick_a_constant_image_stays_constant_under_blur(sigma):
    o = pr.opts(blur_sigma=sigma)
    for level in (0, 1, 40, 215, 255):
        src = np.full((1, 9, 14), level, dtype=np.uint8)
        assert np.array_equal(pr.apply(src, np.uint8, pr.tables(o), o), src)
        assert np.array_equal(pr.apply(src, np.uint16, pr.tables(o), o), src.astype(np.uint16) * 257)


def test_yardstick_draws_have_zero_mean_and_unit_variance():
    z = pr.draws(12345, 400, 250)                                        # 10^5 pixels
    assert z.size == 100000
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02, (z.mean(), z.std())
    assert np.abs(z).max() <= 6.0
    assert np.array_equal(z, pr.draws(12345 + (1 << 64), 400, 250))      # modulo 2^64


def test_yardstick_two_seeds_differ_and_image_k_is_image_0_of_first_index_k():
    src = _random(np.uint8, n=4)
    o = pr.opts(noise_read=3.0, noise_shot=0.1, seed=9)
    a = pr.apply(src, np.uint8, pr.tables(o), o)
    b = pr.apply(src, np.uint8, pr.tables(o), dict(o, seed=10))
    assert not np.array_equal(a, b)
    for k in range(4):
        alone = pr.apply(src[k:k + 1], np.uint8, pr.tables(o), dict(o, first_index=k))
        assert np.array_equal(alone[0], a[k]), k
    assert not np.array_equal(a[0], pr.apply(src[:1], np.uint8, pr.tables(o), dict(o, first_index=1))[0])


def test_yardstick_mix_is_splitmix64s_finaliser():
    """splitmix64 from the state 0: its first outputs are the finaliser of 1, 2, 3 times the golden gamma (the published test vector)."""
    gamma = 0x9E3779B97F4A7C15
    state = np.array([(gamma * k) & ((1 << 64) - 1) for k in (1, 2, 3)], dtype=np.uint64)
    assert [int(v) for v in pr.mix(state)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


# ---- every argument error that needs no device --------------------------------------------------------------------------------------------
BAD_OPTS = [(dict(blur_sigma=-1e-9), "blur_sigma"), (dict(blur_sigma=5.34), "blur_sigma"), (dict(blur_sigma=float("nan")), "blur_sigma"),
            (dict(blur_sigma=float("inf")), "blur_sigma"), (dict(vignette=-0.1), "vignette"), (dict(vignette=float("inf")), "vignette"),
            (dict(vignette=float("nan")), "vignette"), (dict(gain=-1.0), "gain"), (dict(gain=float("inf")), "gain"),
            (dict(gain=float("nan")), "gain"), (dict(noise_read=-1.0), "noise_read"), (dict(noise_read=float("nan")), "noise_read"),
            (dict(noise_shot=-1e-3), "noise_shot"), (dict(noise_shot=float("inf")), "noise_shot"), (dict(first_index=-1), "first_index")]


@pytest.mark.parametrize("kw,word", BAD_OPTS, ids=[f"{list(k)[0]} {list(k.values())[0]}" for k, _ in BAD_OPTS])
def test_tables_refuse_an_option_out_of_range(kw, word):
    lib = _ffi.load()
    r, taps, T = C.c_int32(-7), np.full(17, -3.25), np.full(256, -3.25)
    dp = C.POINTER(C.c_double)
    rc = lib.ccal_photo_tables(C.byref(_ffi.PhotoOpts(**pr.opts(**kw))), C.byref(r), taps.ctypes.data_as(dp), T.ctypes.data_as(dp))
    assert rc == _ffi.ERR_INVALID_ARG
    assert r.value == -7 and (taps == -3.25).all() and (T == -3.25).all()
    with pytest.raises(ValueError):
        engine.photo_tables(api.PhotoOpts(**pr.opts(**kw)))


def test_null_arguments():
    """What is refused before a context is looked at: a NULL context in the three device calls, NULL pointers in the host-only two."""
    lib = _ffi.load()
    o = _ffi.PhotoOpts(**pr.opts())
    r, taps, T = C.c_int32(0), np.zeros(17), np.zeros(256)
    dp = C.POINTER(C.c_double)
    args = [C.byref(o), C.byref(r), taps.ctypes.data_as(dp), T.ctypes.data_as(dp)]
    assert lib.ccal_photo_tables(*args) == _ffi.OK
    for k in range(4):
        assert lib.ccal_photo_tables(*[None if j == k else a for j, a in enumerate(args)]) == _ffi.ERR_INVALID_ARG, k
    INV = _ffi.ERR_INVALID_ARG
    assert lib.ccal_photo_apply_dev(None, _ffi.PIX_U8, _ffi.PIX_U8, 8, 8, 1, None, None, C.byref(o)) == INV
    assert lib.ccal_render_photo_targets(None, 0, None, _ffi.PIX_U8, 8, 8, 0, None, None, None, C.byref(o), None) == INV
    assert lib.ccal_render_photo_targets_dev(None, 0, None, _ffi.PIX_U8, 8, 8, 0, None, None, None, C.byref(o), None) == INV
