"""CPU: the checkerboard assembly's yardstick (tests/board_ref.py, the numpy restatement of the rule include/ccal.h states at
ccal_assemble_checkerboards_batch) against api.assemble_checkerboard on every input the host function is tested with - ids and
positions equal, and positions are copies of inputs, so exactly -, the yardstick's own properties, and the rules of the new entry
points that need no device."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import board_ref  # noqa: E402
import detect_ref as ref  # noqa: E402
from test_detect_cpu import PATTERN, STRAY_SEEDS, _candidates, _inner  # noqa: E402
from camera_intrinsic_calibration_rs_amd import _ffi, api  # noqa: E402

COLS, ROWS = PATTERN
SQ = ref.BOARD_SQUARE


def both(xy, hess, pattern=PATTERN):
    """(the host function's answer, the yardstick's stopped at the first winner)."""
    return api.assemble_checkerboard(xy, hess, pattern, SQ), board_ref.first_winner(xy, hess, pattern[0], pattern[1])


# ---- 1. the yardstick equals api.assemble_checkerboard ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2])
def test_frames_strays_and_input_order(k):
    """The frame, the 40 stray sets of test_spurious_points_and_input_order_change_nothing in their random input orders, and a random
    permutation of the frame."""
    xy, hess = _candidates(k)
    base, mine = both(xy, hess)
    assert base is not None and mine == base
    full = board_ref.assemble(xy, hess, COLS, ROWS)                      # every attempt run: the same board, and its statistics
    assert board_ref.as_dict(full) == base and full["flags"] == 0
    assert full["stats"][0] == 35 and full["stats"][1] >= 1 and full["stats"][2:] == [0, 0]        # the strongest corner's first pair wins
    assert sorted(full["idx"].tolist()) == sorted(set(full["idx"].tolist())) and np.array_equal(xy[full["idx"]], full["xy"])
    inner = np.flatnonzero(_inner(xy, ref.board_frames()[1][k]))
    for seed in STRAY_SEEDS:
        rng = np.random.default_rng(seed)
        extra = []
        while len(extra) < 6:
            p = rng.uniform([6.0, 6.0], [ref.BOARD_W - 7.0, ref.BOARD_H - 7.0])
            if np.abs(np.concatenate([xy, np.array(extra).reshape(-1, 2)]) - p).max(axis=1).min() > 5.0:
                extra.append(p)
        eh = hess[rng.choice(inner, 6)] * rng.uniform(0.8, 1.22, (6, 1))
        order = rng.permutation(len(xy) + 6)
        got, mine = both(np.concatenate([xy, np.array(extra)])[order], np.concatenate([hess, eh])[order])
        assert got == base and mine == base, seed
    perm = np.random.default_rng(40 + k).permutation(len(xy))
    got, mine = both(xy[perm], hess[perm])
    assert got == base and mine == base
    res = board_ref.assemble(xy[perm], hess[perm], COLS, ROWS)
    assert np.array_equal(perm[res["idx"]], full["idx"]) and res["xy"].tobytes() == full["xy"].tobytes()


def test_incomplete_boards_give_none():
    """A lattice corner, an inner corner and the opposite corner dropped, and the wrong pattern: every attempt is run, none wins."""
    xy, hess = _candidates()
    inner = np.flatnonzero(_inner(xy, ref.board_frames()[1][0]))
    for drop in (inner[0], inner[17], inner[-1]):
        keep = np.arange(len(xy)) != drop
        assert both(xy[keep], hess[keep]) == (None, None)
    assert both(xy, hess, (6, 5)) == (None, None)
    assert both(xy[:10], hess[:10]) == (None, None)
    assert both(np.zeros((0, 2)), np.zeros((0, 3))) == (None, None)


def test_square_pattern():
    """5 x 5 corners cut out of the 7 x 5 board: all four rotations are admissible."""
    for k in range(3):
        xy, hess = _candidates(k)
        truth = ref.board_frames()[1][k].reshape(ref.BOARD_ROWS, ref.BOARD_COLS, 2)[:, 1:6].reshape(-1, 2)
        keep = _inner(xy, truth)
        base, mine = both(xy[keep], hess[keep], (5, 5))
        assert base is not None and sorted(base) == list(range(25)) and mine == base


# ---- 2. the yardstick alone -----------------------------------------------------------------------------------------------------------
def synthetic(cols, rows, pitch=20.0, x0=10.0, y0=10.0, strength=100.0):
    """cols x rows ideal saddles on a square grid: hxx = hyy = 0, hxy = +- strength by the cell's parity - the zero-curvature
    directions are the axes, neighbours have opposite polarity."""
    c, r = np.meshgrid(np.arange(cols), np.arange(rows))
    xy = np.stack([x0 + pitch * c.ravel(), y0 + pitch * r.ravel()], axis=1).astype(np.float64)
    hess = np.zeros((cols * rows, 3))
    hess[:, 2] = strength * np.where((c.ravel() + r.ravel()) % 2 == 0, 1.0, -1.0)
    return xy, hess


def test_two_by_two_from_four_synthetic_corners():
    xy, hess = synthetic(2, 2)
    res = board_ref.assemble(xy, hess, 2, 2)
    assert res["found"] == 1 and res["idx"].tolist() == [0, 1, 2, 3] and res["stats"][0] == 4 and res["stats"][2:] == [0, 0]
    assert res["xy"].tolist() == [[10.0, 10.0], [30.0, 10.0], [10.0, 30.0], [30.0, 30.0]]
    back = board_ref.assemble(xy[::-1], hess[::-1], 2, 2)                # the input order changes nothing but idx
    assert back["xy"].tobytes() == res["xy"].tobytes() and back["idx"].tolist() == [3, 2, 1, 0]
    assert api.assemble_checkerboard(xy, hess, (2, 2), SQ) == board_ref.as_dict(res)
    d1, d2 = board_ref.edge_directions(hess)
    a1, a2 = np.abs(d1), np.abs(d2)                                      # one direction along x, the other along y
    assert np.abs(a1 + a2 - 1.0).max() < 1e-15 and np.abs(a1[:, 0] * a1[:, 1]).max() < 1e-15 and np.abs(a1.sum(axis=1) - 1.0).max() < 1e-15


def test_fewer_usable_rows_than_corners():
    xy, hess = synthetic(3, 3)
    res = board_ref.assemble(xy[:8], hess[:8], 3, 3)
    assert (res["found"], res["flags"], res["stats"]) == (0, 0, [0, 0, -1, -1])
    bad = hess.copy()
    bad[4] = [1.0, 1.0, 0.0]                                             # R = -16: not a saddle
    assert board_ref.assemble(xy, bad, 3, 3)["stats"] == [0, 0, -1, -1]
    assert board_ref.assemble(xy, hess, 3, 3)["found"] == 1


def test_unusable_rows_are_ignored():
    """Rows with a NaN or infinite position, R <= 0 or R not finite, anywhere in the input: the same board, idx steps over them."""
    xy, hess = _candidates(1)
    hess = hess.astype(np.float64)
    want = board_ref.assemble(xy, hess, COLS, ROWS)
    junk_xy = np.array([[np.nan, 50.0], [60.0, np.inf], [100.0, 100.0], [120.0, 90.0], [130.0, 95.0]])
    junk_h = np.array([hess[3], hess[4], [5.0, 7.0, 1.0], [0.0, 0.0, 0.0], [np.inf, 1.0, 3.0]])
    at = [0, 7, 7, 30, len(xy)]
    xy2, hess2 = np.insert(xy, at, junk_xy, axis=0), np.insert(hess, at, junk_h, axis=0)
    src = np.insert(np.arange(len(xy)), at, -1)
    got = board_ref.assemble(xy2, hess2, COLS, ROWS)
    assert got["found"] == 1 and got["stats"] == want["stats"] and got["xy"].tobytes() == want["xy"].tobytes()
    assert np.array_equal(src[got["idx"]], want["idx"])


def test_two_identical_positions():
    """A board corner given twice: the copies are at distance 0, which links nothing; one of them fills the cell."""
    xy, hess = _candidates(2)
    want = board_ref.assemble(xy, hess, COLS, ROWS)
    dup = int(want["idx"][17])
    xy2, hess2 = np.concatenate([xy, xy[dup:dup + 1]]), np.concatenate([hess, hess[dup:dup + 1]])
    got = board_ref.assemble(xy2, hess2, COLS, ROWS)
    assert got["found"] == 1 and got["xy"].tobytes() == want["xy"].tobytes() and got["stats"][0] == 36
    assert got["idx"][17] in (dup, len(xy)) and np.array_equal(np.delete(got["idx"], 17), np.delete(want["idx"], 17))
    assert board_ref.as_dict(got) == api.assemble_checkerboard(xy2, hess2, PATTERN, SQ)


def test_the_kept_limit():
    xy, hess = synthetic(27, 19)                                        # 513 rows of one strength: all kept
    assert len(xy) == board_ref.MAX_KEPT + 1
    res = board_ref.assemble(xy, hess, 2, 2)
    assert (res["found"], res["flags"], res["stats"], res["idx"], res["xy"]) == (0, board_ref.FLAG_KEPT_LIMIT, [513, 0, -1, -1], None, None)
    assert len(board_ref.screen(xy[:-1], hess[:-1], 400)[0]) == board_ref.MAX_KEPT      # 512 kept: within the limit
    assert (board_ref.MAX_ROWS, board_ref.MAX_KEPT, board_ref.MIN_SIDE, board_ref.MAX_SIDE) == \
        (_ffi.BOARD_MAX_ROWS, _ffi.BOARD_MAX_KEPT, _ffi.BOARD_MIN_SIDE, _ffi.BOARD_MAX_SIDE)
    assert board_ref.FLAG_KEPT_LIMIT == _ffi.BOARD_FLAG_KEPT_LIMIT


# ---- 3. entry-point rules that need no device ------------------------------------------------------------------------------------------
def test_entry_point_rules_without_a_device():
    lib = _ffi.load()
    IP, DP, LP = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    one, four = np.zeros(1, dtype=np.int32), np.zeros(4, dtype=np.int32)
    xy, offs = np.zeros((4, 2)), np.zeros(2, dtype=np.int64)
    assert lib.ccal_assemble_checkerboards_batch(None, 0, None, None, None, 2, 2, None, None, None, None, None) == _ffi.ERR_INVALID_ARG
    assert lib.ccal_assemble_checkerboards_batch(None, 1, offs.ctypes.data_as(LP), None, None, 2, 2, one.ctypes.data_as(IP),
                                                 xy.ctypes.data_as(DP), None, one.ctypes.data_as(IP), four.ctypes.data_as(IP)) == _ffi.ERR_INVALID_ARG
    o = _ffi.DetectCheckerboardsOpts(step=1, nms_radius=5, min_response=1, rel_q10=102, cand_cap=4096, half_win=5, max_iterations=30,
                                     eps=1e-3, cols=7, rows=5)
    assert ctypes.sizeof(o) == 56
    for fn in (lib.ccal_detect_checkerboards_batch, lib.ccal_detect_checkerboards_dev):
        assert fn(None, 0, 8, 8, 0, None, ctypes.byref(o), None, None, None, None) == _ffi.ERR_INVALID_ARG
        assert fn(None, 0, 8, 8, 1, None, ctypes.byref(o), one.ctypes.data_as(IP), xy.ctypes.data_as(DP), one.ctypes.data_as(IP),
                  None) == _ffi.ERR_INVALID_ARG
    assert not one.any() and not four.any() and not xy.any()
    assert api.detect_checkerboard_points([], PATTERN, SQ, fused=True) == [] == api.detect_checkerboard([], PATTERN, SQ, fused=True)
    img = np.zeros((20, 20), np.uint8)
    for images in ([img, np.zeros((20, 21), np.uint8)], [np.zeros((20, 20, 3), np.uint8)], [np.zeros((20, 20), np.float32)]):
        with pytest.raises(ValueError):
            api.detect_checkerboard(images, PATTERN, SQ, fused=True)
    for pattern, kw in (((1, 5), {}), ((7, 21), {}), (PATTERN, dict(max_per_image=4097)), (PATTERN, dict(max_per_image=0))):
        with pytest.raises(ValueError):
            api.detect_checkerboard_points([img], pattern, SQ, fused=True, **kw)
    with pytest.raises(ValueError):
        api.detect_checkerboard_points([img], PATTERN, 0.0, fused=True)
