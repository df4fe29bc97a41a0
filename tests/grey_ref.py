"""The numpy yardstick of the grey stage (include/ccal.h, "grey frames from colour and raw Bayer frames"; ccal_kernels_grey.hip): the
rule in int64 from the first term to the one rounding.  The GPU tests hold the device to grey() by exact equality.

Also the colour and mosaic frames of the round trips (tests/test_gpu_grey.py): the board fixture of detect_ref tinted and sampled
through a colour filter array, with the worst corner errors the numpy chain (normalize_ref.chain_board) reaches on the yardstick's
grey frames recorded below.  `python tests/grey_ref.py` measures them again (CPU) and prints them beside the recorded constants,
with the raw mosaic fed as grey and a blue tint for comparison (EXPERIMENTS.md)."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

LAYOUTS = ("grey", "rgb", "bgr", "rgba", "bgra", "bayer_rggb", "bayer_bggr", "bayer_grbg", "bayer_gbrg")   # the code is the index
CHANNELS = {"grey": 1, "rgb": 3, "bgr": 3, "rgba": 4, "bgra": 4}
# the (column, row) parity of the R site in the mosaic's 2 x 2 cell; B sits on the opposite corner, G on the other two
BAYER_R = {"bayer_rggb": (0, 0), "bayer_bggr": (1, 1), "bayer_grbg": (1, 0), "bayer_gbrg": (0, 1)}
DEFAULTS = dict(bin=1, w_r=19595, w_g=38470, w_b=7471)


def opts(**kw):
    o = dict(DEFAULTS)
    assert set(kw) <= set(o), kw
    o.update(kw)
    return o


def is_bayer(layout):
    return layout in BAYER_R


def channels(layout):
    return CHANNELS.get(layout, 1)


def out_size(width, height, bin):
    return width // bin, height // bin


def triple4(src, layout):
    """(R4, G4, B4) int64 [n, H, W]: four times the channel values of every source pixel on the 16-bit scale."""
    src = np.asarray(src)
    assert src.dtype in (np.dtype(np.uint8), np.dtype(np.uint16))
    I = src.astype(np.int64) * (257 if src.dtype == np.uint8 else 1)
    if layout == "grey":
        assert I.ndim == 3
        return 4 * I, 4 * I, 4 * I
    if layout in CHANNELS:
        assert I.ndim == 4 and I.shape[3] == CHANNELS[layout]
        r, b = (0, 2) if layout[0] == "r" else (2, 0)
        return 4 * I[..., r], 4 * I[..., 1], 4 * I[..., b]
    n, H, W = I.shape
    assert H >= 2 and W >= 2
    P = np.pad(I, ((0, 0), (1, 1), (1, 1)), mode="reflect")             # -1 -> 1, n -> n - 2: the mosaic's parity is kept
    at = lambda dx, dy: P[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    edge = at(-1, 0) + at(1, 0) + at(0, -1) + at(0, 1)
    diag = at(-1, -1) + at(1, -1) + at(-1, 1) + at(1, 1)
    hor, ver = 2 * (at(-1, 0) + at(1, 0)), 2 * (at(0, -1) + at(0, 1))
    rx, ry = BAYER_R[layout]
    px = ((np.arange(W) & 1) ^ rx)[None, None, :]
    py = ((np.arange(H) & 1) ^ ry)[None, :, None]
    r_site, b_site = (px == 0) & (py == 0), (px == 1) & (py == 1)
    g_in_r_row = (px == 1) & (py == 0)                                     # R to the left and right, B above and below
    G4 = np.where(r_site | b_site, edge, 4 * I)
    R4 = np.where(r_site, 4 * I, np.where(b_site, diag, np.where(g_in_r_row, hor, ver)))
    B4 = np.where(b_site, 4 * I, np.where(r_site, diag, np.where(g_in_r_row, ver, hor)))
    return R4, G4, B4


def grey(src, layout, dst_dtype, o):
    """src [n, H, W] (grey and Bayer layouts) or [n, H, W, c] (interleaved) of uint8 / uint16 by the rule with the options o
    (bin, w_r, w_g, w_b): the images [n, H // bin, W // bin] of dst_dtype."""
    b, w = int(o["bin"]), (int(o["w_r"]), int(o["w_g"]), int(o["w_b"]))
    assert b in (1, 2, 4) and min(w) >= 0 and sum(w) == 65536
    R4, G4, B4 = triple4(src, layout)
    N = w[0] * R4 + w[1] * G4 + w[2] * B4
    assert int(N.max(initial=0)) < 2 ** 34
    n, H, W = N.shape
    Wo, Ho = out_size(W, H, b)
    assert Wo >= 1 and Ho >= 1
    S = N[:, :Ho * b, :Wo * b].reshape(n, Ho, b, Wo, b).sum(axis=(2, 4))
    s = 18 + 2 * {1: 0, 2: 1, 4: 2}[b]
    if np.dtype(dst_dtype) == np.uint16:
        return ((S + (1 << (s - 1))) >> s).astype(np.uint16)
    return ((S + 257 * (1 << (s - 1))) // (257 * (1 << s))).astype(np.uint8)


# ---- the cases of tests/test_gpu_grey.py: blocks through ccal_grey_dev --------------------------------------------------------------------
def _case(name, layout, src, dst, n, height, width, kind="random", **o):
    return {"name": name, "layout": layout, "src": np.dtype(src), "dst": np.dtype(dst), "n": n, "height": height, "width": width,
            "kind": kind, "opts": opts(**o)}


def _random_weights(seed):
    rng = np.random.default_rng(seed)
    a, b = sorted(int(v) for v in rng.integers(0, 65537, 2))
    return dict(w_r=a, w_g=b - a, w_b=65536 - b)


@functools.lru_cache(maxsize=None)
def parity_cases():
    """All nine layouts x the four type pairs x bins 1, 2, 4 at 67 x 45 (201-byte u8 RGB rows, u16 rows off a dword; 33 x 22 and
    16 x 11 out, remainders dropped); 1 x 1 for the five layouts without a mosaic; 2 x 2, 3 x 2, 2 x 3, a 2-wide column of height 45
    and 4 x 4 at bin 4 for the four mosaics; 130 x 67 (several tiles each way, halo across their seams); 65 images of 9 x 5 and
    70 000 images of 2 x 2 RGGB (more than the grid's image axis holds); full-scale frames for every layout at bin 4 to u16 (the largest
    S); the weights (65536, 0, 0), (0, 0, 65536) and random ones."""
    u8, u16 = np.uint8, np.uint16
    short = lambda t: "u8" if t == u8 else "u16"
    cases = []
    for layout in LAYOUTS:
        for s in (u8, u16):
            for d in (u8, u16):
                for b in (1, 2, 4):
                    cases.append(_case(f"67 x 45 {layout} {short(s)} to {short(d)} bin {b}", layout, s, d, 2, 45, 67, bin=b))
    for k, layout in enumerate(LAYOUTS[:5]):
        cases.append(_case(f"1 x 1 {layout}", layout, (u8, u16)[k & 1], (u16, u8, u8, u16, u16)[k], 3, 1, 1))
    for k, layout in enumerate(LAYOUTS[5:]):
        s, d = (u8, u16)[k & 1], (u8, u16)[(k >> 1) & 1]
        cases.append(_case(f"2 x 2 {layout}", layout, s, d, 3, 2, 2))
        cases.append(_case(f"2 x 2 {layout} bin 2", layout, d, s, 3, 2, 2, bin=2))
        cases.append(_case(f"3 x 2 {layout}", layout, d, d, 2, 2, 3))
        cases.append(_case(f"2 x 3 {layout}", layout, s, s, 2, 3, 2))
        cases.append(_case(f"2 x 45 column {layout}", layout, s, d, 1, 45, 2, bin=(1, 2)[k & 1]))
        cases.append(_case(f"4 x 4 {layout} bin 4", layout, d, s, 2, 4, 4, bin=4))
    for layout, s, d, b in (("grey", u8, u8, 1), ("rgb", u8, u8, 1), ("rgb", u16, u16, 2), ("bgra", u8, u16, 4), ("rgba", u16, u8, 1),
                            ("bayer_rggb", u8, u8, 1), ("bayer_gbrg", u16, u16, 2), ("bayer_grbg", u8, u16, 4), ("bayer_bggr", u16, u8, 1)):
        cases.append(_case(f"130 x 67 {layout} {short(s)} to {short(d)} bin {b}", layout, s, d, 2, 67, 130, bin=b))
    cases.append(_case("65 images 9 x 5 rgb", "rgb", u8, u16, 65, 5, 9))
    cases.append(_case("65 images 9 x 5 bayer_grbg", "bayer_grbg", u16, u8, 65, 5, 9, bin=2))
    cases.append(_case("70000 images 2 x 2 bayer_rggb", "bayer_rggb", u8, u8, 70000, 2, 2))
    for layout in LAYOUTS:
        cases.append(_case(f"full scale {layout} u16 bin 4", layout, u16, u16, 1, 45, 67, kind="full", bin=4))
        cases.append(_case(f"full scale {layout} u8 bin 4", layout, u8, u16, 1, 45, 67, kind="full", bin=4))
        cases.append(_case(f"full scale {layout} u16 to u8 bin 4", layout, u16, u8, 1, 45, 67, kind="full", bin=4))
    for k, (layout, s, d, b) in enumerate((("rgb", u8, u8, 1), ("bgra", u16, u16, 2), ("bayer_rggb", u16, u8, 1), ("bayer_gbrg", u8, u16, 4))):
        cases.append(_case(f"weights red only {layout}", layout, s, d, 1, 45, 67, bin=b, w_r=65536, w_g=0, w_b=0))
        cases.append(_case(f"weights blue only {layout}", layout, s, d, 1, 45, 67, bin=b, w_r=0, w_g=0, w_b=65536))
        cases.append(_case(f"weights random {layout}", layout, s, d, 1, 45, 67, bin=b, **_random_weights(100 + k)))
    assert len({c["name"] for c in cases}) == len(cases)
    return tuple(cases)


def source(case):
    """The source block of a case: random over the whole range of its type, or full scale."""
    n, H, W = case["n"], case["height"], case["width"]
    c = channels(case["layout"])
    shape = (n, H, W) if c == 1 else (n, H, W, c)
    hi = np.iinfo(case["src"]).max
    if case["kind"] == "full":
        return np.full(shape, hi, dtype=case["src"])
    rng = np.random.default_rng(sum(map(ord, case["name"])))
    return rng.integers(0, hi + 1, shape).astype(case["src"])


# ---- round trips: the board fixture as a colour frame and as a mosaic ---------------------------------------------------------------------
# Frame 0 of detect_ref.BOARD_FRAMES: the 7 x 5 board in a 320 x 240 image under Camera(400, 159.5, 119.5, 0).  The "large" frame is the
# same board and pose seen by a 640 x 480 camera of twice the focal length (Camera(800, 319.5, 239.5, 0)): binned by 2 it is the
# small frame's view, a true corner (x, y) of the large frame lying at ((x - 0.5) / 2, (y - 0.5) / 2) of the binned one.  A tint
# (t_r, t_g, t_b) makes the colour frame rint(t_c g) of the uint8 grey frame g; a mosaic keeps of every pixel the channel of its site.
# Per case: (name, large frame, tint, layout, bin).  RT_WORST: the worst distance (px) from the true corner that the numpy chain
# (normalize_ref.chain_board) reaches on grey(...) of the case's uint8 source to uint8; the GPU round trips are held to 1.5 x that
# (rt_bound; the project's convention, detect_ref.BOARD_BOUND).
RT_CASES = (
    ("a", False, (1.0, 0.85, 0.6), "rgb", 1),
    ("b", False, (1.0, 0.85, 0.6), "bayer_rggb", 1),
    ("c", True, (1.0, 0.45, 0.15), "rgb", 2),
    ("d", True, (1.0, 0.45, 0.15), "bayer_rggb", 2),
    ("e", True, (1.0, 0.45, 0.15), "bayer_gbrg", 2),
)
RT_WORST = (0.08234, 0.15415, 0.06144, 0.10597, 0.09631)
# for comparison, measured by the script only: the untinted frame 0.08148 px, the untinted large frame binned by 2 0.06026 px


def rt_bound(worst):
    return 1.5 * worst


@functools.lru_cache(maxsize=None)
def board_frame(large):
    """(the uint8 grey frame, the true corner pixels [35, 2]) of the fixture's frame 0, at 320 x 240 or, large, at 640 x 480 and twice
    the focal length."""
    import detect_ref as dr
    k = 2 if large else 1
    lam, rot, tilt, axis, centre = dr.BOARD_FRAMES[0]
    W, H = k * dr.BOARD_W, k * dr.BOARD_H
    cam = dr.Camera(k * dr.BOARD_F, (W - 1) / 2.0, (H - 1) / 2.0, lam)
    R, t = dr.board_pose(dr.BOARD_COLS, dr.BOARD_ROWS, dr.BOARD_SQUARE, rot, tilt, axis, centre)
    img, truth = dr.render_board(W, H, cam, R, t, dr.BOARD_COLS, dr.BOARD_ROWS, dr.BOARD_SQUARE, np.uint8)
    img.setflags(write=False)
    return img, truth


def tinted(img, tint):
    """The RGB frame [H, W, 3] of the grey frame under the tint."""
    return np.rint(img[..., None].astype(np.float64) * np.asarray(tint, dtype=np.float64)).astype(img.dtype)


def mosaic(rgb, layout):
    """The raw frame [H, W] a sensor with the colour filter array `layout` records of the RGB frame."""
    H, W, _ = rgb.shape
    rx, ry = BAYER_R[layout]
    px, py = ((np.arange(W) & 1) ^ rx)[None, :], ((np.arange(H) & 1) ^ ry)[:, None]
    ch = np.where((px == 0) & (py == 0), 0, np.where((px == 1) & (py == 1), 2, 1))
    return np.take_along_axis(rgb, ch[..., None], axis=2)[..., 0]


def rt_source(k, tint=None):
    """Round trip k: (the uint8 source frame - [H, W, 3] or [H, W] -, the layout, the bin, the true corners in the output frame)."""
    _, large, t, layout, b = RT_CASES[k]
    img, truth = board_frame(large)
    rgb = tinted(img, t if tint is None else tint)
    src = mosaic(rgb, layout) if is_bayer(layout) else rgb
    return src, layout, b, (truth - (b - 1) / 2.0) / b


def rt_grey(k, tint=None):
    """The yardstick's uint8 grey frame of round trip k, and the true corners in it."""
    src, layout, b, truth = rt_source(k, tint)
    return grey(src[None], layout, np.uint8, opts(bin=b))[0], truth


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import normalize_ref as nr

    def err(img, truth):
        xy = nr.chain_board(np.ascontiguousarray(img))
        return "None" if xy is None else f"{nr.board_error(xy, truth):.5f}"

    for large in (False, True):
        img, truth = board_frame(large)
        if large:
            print(f"untinted large frame binned by 2: {err(grey(img[None], 'grey', np.uint8, opts(bin=2))[0], (truth - 0.5) / 2.0)} px", flush=True)
        else:
            print(f"untinted frame: {err(img, truth)} px", flush=True)
    for k, case in enumerate(RT_CASES):
        g, truth = rt_grey(k)
        print(f"case {case}: worst corner error {err(g, truth)} px (recorded {RT_WORST[k]})", flush=True)
    # a raw mosaic fed as grey against its bin-1 demosaic, for a warm, a strong warm and a blue tint (EXPERIMENTS.md)
    img, truth = board_frame(False)
    for tint in ((1.0, 0.85, 0.6), (1.0, 0.45, 0.15), (0.3, 0.6, 1.0)):
        for layout in LAYOUTS[5:]:
            raw = mosaic(tinted(img, tint), layout)
            print(f"tint {tint} {layout}: raw mosaic as grey {err(raw, truth)} px, bin-1 demosaic "
                  f"{err(grey(raw[None], layout, np.uint8, opts())[0], truth)} px", flush=True)
