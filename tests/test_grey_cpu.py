"""CPU: the grey stage (ccal_grey_dev; ccal_kernels_grey.hip) without a GPU.  The consequences that include/ccal.h states of the rule,
on tests/grey_ref.py, its numpy yardstick; that the case list of tests/test_gpu_grey.py covers what it claims; the argument check
(csrc/ccal_image_plan.hpp: grey_stage_check) through a plain C++ program (tests/cpp/test_grey_check.cpp) under the host's address and
undefined-behaviour sanitizers; the compiler's resource remark for every kernel of the unit; the bindings."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grey_ref as gr  # noqa: E402

from camera_intrinsic_calibration_rs_amd import _ffi, api, engine  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
U8, U16 = np.dtype(np.uint8), np.dtype(np.uint16)
BINS = (1, 2, 4)


def _random(layout, dtype, n=2, H=13, W=18, seed=5):
    c = gr.channels(layout)
    shape = (n, H, W) if c == 1 else (n, H, W, c)
    return np.random.default_rng(seed).integers(0, np.iinfo(dtype).max + 1, shape).astype(dtype)


# ---- the consequences of the rule ----------------------------------------------------------------------------------------------------------
def test_grey_at_bin_1_is_a_copy_or_the_change_of_scale():
    for dtype in (U8, U16):
        src = _random("grey", dtype)
        assert np.array_equal(gr.grey(src, "grey", dtype, gr.opts()), src)
    p = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)
    assert np.array_equal(gr.grey(p, "grey", U16, gr.opts()), p.astype(np.uint16) * 257)
    v = np.arange(65536, dtype=np.uint16).reshape(1, 256, 256)
    assert np.array_equal(gr.grey(v, "grey", U8, gr.opts()), ((v.astype(np.int64) + 128) // 257).astype(np.uint8))


@pytest.mark.parametrize("layout", gr.LAYOUTS)
def test_u8_and_257_times_u16_sources_give_equal_output(layout):
    src = _random(layout, U8)
    wide = src.astype(np.uint16) * np.uint16(257)
    for b in BINS:
        for dst in (U8, U16):
            for w in (gr.opts(bin=b), gr.opts(bin=b, w_r=1, w_g=2, w_b=65533)):
                assert np.array_equal(gr.grey(src, layout, dst, w), gr.grey(wide, layout, dst, w)), (b, dst)


@pytest.mark.parametrize("layout", gr.LAYOUTS[5:])
def test_a_constant_mosaic_gives_its_value(layout):
    for dtype, v in ((U8, 0x5B), (U16, 0x5B17), (U16, 1), (U8, 254)):
        for H, W in ((2, 2), (3, 2), (2, 3), (9, 12)):
            src = np.full((1, H, W), v, dtype=dtype)
            for b in (b for b in BINS if b <= min(H, W)):
                assert (gr.grey(src, layout, dtype, gr.opts(bin=b)) == v).all(), (dtype, v, H, W, b)


@pytest.mark.parametrize("layout", gr.LAYOUTS)
def test_full_scale_gives_full_scale_at_every_bin(layout):
    c = gr.channels(layout)
    for dtype in (U8, U16):
        src = np.full((1, 9, 12) if c == 1 else (1, 9, 12, c), np.iinfo(dtype).max, dtype=dtype)
        for b in BINS:
            assert (gr.grey(src, layout, U8, gr.opts(bin=b)) == 255).all() and (gr.grey(src, layout, U16, gr.opts(bin=b)) == 65535).all()
            for w in ((65536, 0, 0), (0, 65536, 0), (0, 0, 65536)):
                assert (gr.grey(src, layout, U16, gr.opts(bin=b, w_r=w[0], w_g=w[1], w_b=w[2])) == 65535).all()
            assert not gr.grey(np.zeros_like(src), layout, U16, gr.opts(bin=b)).any()


def test_bgr_is_rgb_with_the_channels_swapped_and_alpha_is_ignored():
    for dtype in (U8, U16):
        rgb = _random("rgb", dtype)
        alpha = _random("grey", dtype, seed=6)
        for b in BINS:
            o = gr.opts(bin=b)
            want = gr.grey(rgb, "rgb", dtype, o)
            assert np.array_equal(gr.grey(rgb[..., ::-1], "bgr", dtype, o), want)
            for a in (alpha, np.zeros_like(alpha)):
                rgba = np.concatenate([rgb, a[..., None]], axis=3)
                bgra = np.concatenate([rgb[..., ::-1], a[..., None]], axis=3)
                assert np.array_equal(gr.grey(rgba, "rgba", dtype, o), want) and np.array_equal(gr.grey(bgra, "bgra", dtype, o), want)
            # and BGR with w_r and w_b exchanged is RGB on the same block: how the kernel does it
            assert np.array_equal(gr.grey(rgb, "bgr", dtype, gr.opts(bin=b, w_r=o["w_b"], w_b=o["w_r"])), want)


def test_a_mosaic_of_a_grey_frame_and_the_four_mosaics_of_one_colour_frame():
    """A mosaic whose three channels are equal is the grey frame itself away from nothing - the interpolation of a constant-colour
    region is exact - and the four layouts see the same scene: on a frame of one colour they agree with the RGB rule."""
    rgb = np.broadcast_to(np.array([200, 90, 30], dtype=np.uint8), (1, 10, 12, 3)).copy()
    want = gr.grey(rgb, "rgb", U16, gr.opts())
    for layout in gr.LAYOUTS[5:]:
        raw = gr.mosaic(rgb[0], layout)[None]
        assert np.array_equal(gr.grey(raw, layout, U16, gr.opts()), want), layout
    # the table of include/ccal.h: the cell at the origin, row-major
    cell = np.array([[[10, 20, 30]]], dtype=np.uint8).repeat(2, 0).repeat(2, 1)
    assert [gr.mosaic(cell, l).reshape(-1).tolist() for l in gr.LAYOUTS[5:]] == [[10, 20, 20, 30], [30, 20, 20, 10], [20, 10, 30, 20], [20, 30, 10, 20]]


def test_the_mosaic_rule_term_by_term():
    """One 4 x 4 RGGB frame by hand: an R site in the middle, a G site on the border, the reflected corner."""
    I = (np.arange(16, dtype=np.int64).reshape(4, 4) * 7 + 3).astype(np.uint16)
    R4, G4, B4 = (t[0] for t in gr.triple4(I[None], "bayer_rggb"))
    v = I.astype(np.int64)
    # (2, 2) is an R site: edge neighbours are G, diagonal ones B
    assert R4[2, 2] == 4 * v[2, 2] and G4[2, 2] == v[2, 1] + v[2, 3] + v[1, 2] + v[3, 2] and B4[2, 2] == v[1, 1] + v[1, 3] + v[3, 1] + v[3, 3]
    # (x, y) = (1, 0) is a G site in an R row: R left and right, B above and below, the row above reflected to row 1
    assert G4[0, 1] == 4 * v[0, 1] and R4[0, 1] == 2 * (v[0, 0] + v[0, 2]) and B4[0, 1] == 2 * (v[1, 1] + v[1, 1])
    # (0, 0) is an R site in the corner: -1 reflects to 1 both ways
    assert G4[0, 0] == 2 * v[0, 1] + 2 * v[1, 0] and B4[0, 0] == 4 * v[1, 1]
    # (3, 3) is a B site in the far corner: 4 reflects to 2
    assert B4[3, 3] == 4 * v[3, 3] and G4[3, 3] == 2 * v[3, 2] + 2 * v[2, 3] and R4[3, 3] == 4 * v[2, 2]


def test_binning_sums_the_blocks_and_rounds_once():
    src = _random("rgb", U16, n=1, H=9, W=11)
    N = sum(w * t for w, t in zip((19595, 38470, 7471), gr.triple4(src, "rgb")))
    for b, s in ((1, 18), (2, 20), (4, 22)):
        Wo, Ho = gr.out_size(11, 9, b)
        got16, got8 = gr.grey(src, "rgb", U16, gr.opts(bin=b)), gr.grey(src, "rgb", U8, gr.opts(bin=b))
        assert got16.shape == (1, Ho, Wo)
        for Y in range(Ho):
            for X in range(Wo):
                S = int(N[0, Y * b:(Y + 1) * b, X * b:(X + 1) * b].sum())
                assert got16[0, Y, X] == (S + (1 << (s - 1))) >> s and got8[0, Y, X] == (S + 257 * (1 << (s - 1))) // (257 << s)
    # half up: S = 2^(s-1) exactly (R = 1: R4 = 4, N = 4 x 32768 = 2^17) gives 1, four less gives 0
    one = np.zeros((1, 1, 1, 3), dtype=np.uint16); one[..., 0] = 1
    assert gr.grey(one, "rgb", U16, dict(bin=1, w_r=32768, w_g=32768, w_b=0))[0, 0, 0] == 1
    assert gr.grey(one, "rgb", U16, dict(bin=1, w_r=32767, w_g=32769, w_b=0))[0, 0, 0] == 0


def test_an_image_does_not_depend_on_its_batch():
    for layout in ("rgb", "bayer_grbg"):
        src = _random(layout, U8, n=5)
        whole = gr.grey(src, layout, U16, gr.opts(bin=2))
        for k in range(5):
            assert np.array_equal(gr.grey(src[k:k + 1], layout, U16, gr.opts(bin=2))[0], whole[k])


# ---- the cases of the GPU tests ------------------------------------------------------------------------------------------------------------
def test_the_cases_cover_what_they_claim():
    cases = gr.parity_cases()
    pairs = {(a, b) for a in ("uint8", "uint16") for b in ("uint8", "uint16")}
    at = lambda w, h: [c for c in cases if (c["width"], c["height"]) == (w, h) and c["kind"] == "random"]
    combos = {(c["layout"], c["src"].name, c["dst"].name, c["opts"]["bin"]) for c in at(67, 45)}
    assert combos >= {(l, s, d, b) for l in gr.LAYOUTS for (s, d) in pairs for b in BINS}
    assert {gr.out_size(67, 45, b) for b in BINS} == {(67, 45), (33, 22), (16, 11)}
    assert {c["layout"] for c in at(1, 1)} == set(gr.LAYOUTS[:5])
    for shape in ((2, 2), (3, 2), (2, 3), (2, 45)):
        assert {c["layout"] for c in at(*shape)} >= set(gr.LAYOUTS[5:]), shape
    assert {c["layout"] for c in at(4, 4) if c["opts"]["bin"] == 4} == set(gr.LAYOUTS[5:])
    wide = at(130, 67)
    assert {c["opts"]["bin"] for c in wide} == set(BINS) and {(c["src"].name, c["dst"].name) for c in wide} == pairs
    assert sum(gr.is_bayer(c["layout"]) for c in wide) >= 4 and {"grey", "rgb", "rgba", "bgra"} <= {c["layout"] for c in wide}
    assert any(c["n"] == 65 for c in cases) and any(c["n"] > 65535 and c["layout"] == "bayer_rggb" and (c["width"], c["height"]) == (2, 2) for c in cases)
    full = [c for c in cases if c["kind"] == "full" and c["opts"]["bin"] == 4 and c["src"] == U16 and c["dst"] == U16]
    assert {c["layout"] for c in full} == set(gr.LAYOUTS)
    for c in full:
        assert (gr.grey(gr.source(c), c["layout"], c["dst"], c["opts"]) == 65535).all()
    w = {(c["opts"]["w_r"], c["opts"]["w_g"], c["opts"]["w_b"]) for c in cases}
    assert (65536, 0, 0) in w and (0, 0, 65536) in w and len(w) >= 7 and all(sum(t) == 65536 and min(t) >= 0 for t in w)
    for c in cases:
        assert gr.source(c).dtype == c["src"] and gr.source(c).shape[:3] == (c["n"], c["height"], c["width"])
    # the random sources reach both ends of their type, so that every weight and shift is exercised on large terms
    big = gr.source(next(c for c in cases if c["name"] == "130 x 67 rgb u16 to u16 bin 2"))
    assert big.min() < 64 and big.max() > 65535 - 64


def test_the_round_trip_frames_are_what_they_claim():
    img, truth = gr.board_frame(False)
    big, big_truth = gr.board_frame(True)
    assert img.shape == (240, 320) and big.shape == (480, 640) and truth.shape == (35, 2)
    assert np.abs((big_truth - 0.5) / 2.0 - truth).max() < 1e-9             # the large camera binned by 2 is the small one
    src, layout, b, _ = gr.rt_source(0)
    assert src.shape == (240, 320, 3) and src.dtype == np.uint8 and (layout, b) == ("rgb", 1)
    assert np.array_equal(src[..., 0], img) and src[..., 2].max() == round(0.6 * int(img.max()))
    raw, layout, b, _ = gr.rt_source(3)
    assert raw.shape == (480, 640) and (layout, b) == ("bayer_rggb", 2)
    rgb = gr.tinted(big, (1.0, 0.45, 0.15))
    assert np.array_equal(raw[0::2, 0::2], rgb[0::2, 0::2, 0]) and np.array_equal(raw[1::2, 1::2], rgb[1::2, 1::2, 2])
    assert np.array_equal(raw[0::2, 1::2], rgb[0::2, 1::2, 1])
    assert len(gr.RT_WORST) == len(gr.RT_CASES) == 5 and all(0.0 < w < 0.25 for w in gr.RT_WORST)


# ---- the argument check, under the host's sanitizers ---------------------------------------------------------------------------------------
def test_the_stage_check_gives_each_message_in_its_order(tmp_path):
    exe = str(tmp_path / "test_grey_check")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Xarch_host", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "test_grey_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.stdout[-4000:], out.stderr[-4000:])
    # the program counts what it checked: 108 good calls, 38 on single messages, 6 on the pixel count, 14 on the order, 16 on
    # n_img == 0, 120 + 4 on overlap
    assert out.stdout.strip() == "OK 306", out.stdout[-2000:]


# ---- the kernels -----------------------------------------------------------------------------------------------------------------------------
def test_the_grey_kernels_need_no_scratch(tmp_path):
    """The compiler's resource remark for gfx950: ScratchSize 0 for every instantiation of k_grey (2 source types x 2 destination
    types x 3 bins x 4 kinds of pixel), and every one of them is there."""
    csrc = os.path.join(ROOT, "camera_intrinsic_calibration_rs_amd", "csrc")
    r = subprocess.run([os.environ.get("HIPCC", HIPCC), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=fast", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "ccal_kernels_grey.hip"),
                        "-o", str(tmp_path / "grey.out")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == 48 and len(set(names)) == 48 and all("k_grey" in n for n in names), names
    assert scratch == [0] * 48, list(zip(names, scratch))


def test_the_unit_uses_no_floating_point_and_no_atomics():
    src = open(os.path.join(ROOT, "camera_intrinsic_calibration_rs_amd", "csrc", "ccal_kernels_grey.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"\b(double|float|atomic\w*)\b", code)
    make = open(os.path.join(ROOT, "camera_intrinsic_calibration_rs_amd", "csrc", "Makefile")).read()
    assert "ccal_kernels_grey" not in make                                  # the wildcard picks it up; no -ffp-contract line


# ---- the bindings ----------------------------------------------------------------------------------------------------------------------------
def test_the_bindings():
    import ctypes as C
    lib = _ffi.load()
    o = _ffi.GreyOpts()
    assert lib.ccal_grey_set_defaults(C.byref(o)) == _ffi.OK and (o.bin, o.w_r, o.w_g, o.w_b) == (1, 19595, 38470, 7471)
    assert lib.ccal_grey_set_defaults(None) == _ffi.ERR_INVALID_ARG
    assert C.sizeof(_ffi.GreyOpts) == 16
    d = api.GreyOpts()
    assert (d.bin, d.w_r, d.w_g, d.w_b) == (1, 19595, 38470, 7471) == tuple(gr.DEFAULTS[k] for k in ("bin", "w_r", "w_g", "w_b"))
    o = engine.grey_opts(api.GreyOpts(bin=4, w_r=65536, w_g=0, w_b=0))
    assert (o.bin, o.w_r, o.w_g, o.w_b) == (4, 65536, 0, 0) and engine.grey_opts(o) is o
    assert list(api.LAYOUTS) == list(gr.LAYOUTS) and list(api.LAYOUTS.values()) == list(range(9))
    assert (_ffi.LAYOUT_GREY, _ffi.LAYOUT_RGB, _ffi.LAYOUT_BGRA, _ffi.LAYOUT_BAYER_RGGB, _ffi.LAYOUT_BAYER_GBRG) == (0, 1, 4, 5, 8)
    header = open(os.path.join(ROOT, "include", "ccal.h")).read()
    enum = re.search(r"typedef enum \{([^}]*)\} ccal_pixel_layout;", header, flags=re.S).group(1)
    assert [n.split("=")[0].strip().replace("CCAL_LAYOUT_", "").lower() for n in enum.split(",")] == list(gr.LAYOUTS)
    assert engine.grey_out_size(67, 45, 1) == (67, 45) and engine.grey_out_size(67, 45, 2) == (33, 22) and engine.grey_out_size(67, 45, 4) == (16, 11)
    assert ccal_grey_dev_needs_a_context(lib)


def ccal_grey_dev_needs_a_context(lib):
    import ctypes as C
    o = _ffi.GreyOpts(bin=1, w_r=19595, w_g=38470, w_b=7471)
    return lib.ccal_grey_dev(None, _ffi.LAYOUT_RGB, _ffi.PIX_U8, _ffi.PIX_U8, 8, 8, 0, None, None, C.byref(o)) == _ffi.ERR_INVALID_ARG
