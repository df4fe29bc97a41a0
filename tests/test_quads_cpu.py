"""CPU: the quad proposer's rule as tests/quad_ref.py restates it (the yardstick the GPU tests hold the kernels to) - end to end
through the four yardsticks on the rendered AprilGrid fixture, the rule's cases one by one, the merge of api.propose_quads, the
constants of the binding against the header, and the margin condition of every fixture the GPU parity tests use.  No GPU, nothing
outside the repository."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quad_ref as ref  # noqa: E402
import tag_ref  # noqa: E402

from camera_intrinsic_calibration_rs_amd import _ffi, api  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the binding's constants --------------------------------------------------------------------------------------------------------
def test_constants_are_the_headers():
    src = open(os.path.join(ROOT, "include", "ccal.h")).read()
    assert int(re.search(r"#define CCAL_QUAD_MAX_OUT_EDGES (\d+)", src).group(1)) == _ffi.QUAD_MAX_OUT_EDGES == ref.MAX_OUT_EDGES
    assert _ffi.QUAD_FLAG_CUT == ref.FLAG_CUT == 1
    # what the rule reports for arguments it does not accept: CCAL_ERR_INVALID_ARG, the status the binding calls ERR_INVALID_ARG
    body = re.search(r"typedef enum \{([^}]*)\} ccal_status;", src, flags=re.S).group(1)
    status = {k: int(v) for k, v in re.findall(r"(CCAL_[A-Z_]+)\s*=\s*(\d+)", body)}
    assert status["CCAL_ERR_INVALID_ARG"] == _ffi.ERR_INVALID_ARG == 1 and status["CCAL_OK"] == _ffi.OK == 0
    assert _ffi.STATUS_NAMES[_ffi.ERR_INVALID_ARG] == "CCAL_ERR_INVALID_ARG"
    text = re.search(r"proposing AprilGrid tag quads.*?#define CCAL_QUAD_MAX_OUT_EDGES", src, flags=re.S).group(0)
    assert "CCAL_ERR_INVALID_ARG, nothing launched or written" in text and "32768" in text
    for name in ("ccal_propose_quads_batch", "ccal_propose_quads_dev"):
        assert [s for s in _ffi.SYMBOLS if s[0] == name]


# ---- end to end through the four yardsticks -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_the_fixture_through_the_four_yardsticks(dtype):
    """detect_ref -> corner_ref -> quad_ref -> tag_ref on tag_ref.grid_frames at nms_radius 5: exactly the six tag outlines per
    frame, within 0.2 px of the projected truth up to a cyclic shift, ids 0 .. 5 at Hamming distance 0, no list cut.  With
    min_side 6 the twelve gap squares are proposed as well, and the decoder rejects them by their border."""
    scale = 257 if dtype == np.uint16 else 1
    imgs, truth = tag_ref.grid_frames(dtype)
    codes = tag_ref.grid_family().codes
    for min_side, want in ((20.0, 6), (6.0, 18)):
        case = ref.fixture_case(dtype, min_side)
        worst = 0.0
        for k, r in enumerate(ref.yardstick(case)):
            assert (r["count"], r["flags"]) == (want, 0), (k, min_side)
            ids, extra = [], 0
            for q in r["quads"]:
                hit = [m for m in range(6) if ref.same_outline(q, truth[k][m], 0.2)]
                d = tag_ref.decode_one(imgs[k], q, tag_ref.GRID_D, tag_ref.GRID_BORDER, codes, 3, 20.0 * scale, 0, 2)
                if hit:
                    assert (d["reason"], d["id"], d["hamming"]) == (tag_ref.OK, hit[0], 0), (k, hit)
                    ids.append(hit[0])
                    worst = max(worst, min(np.linalg.norm(np.roll(q, -s, axis=0) - truth[k][hit[0]], axis=1).max() for s in range(4)))
                else:
                    assert d["reason"] == tag_ref.BORDER, (k, tag_ref.REASONS[d["reason"]])
                    extra += 1
            assert sorted(ids) == list(range(6)) and extra == want - 6
        print(f"{np.dtype(dtype).name} min_side {min_side:g}: worst corner distance to the truth {worst:.4f} px")


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_a_frame_cropped_to_four_tags_on_the_cpu(dtype):
    """The crop the GPU end-to-end test hands to api.detect_aprilgrid (frame 0 cut through the middle of its right tag column):
    the chain of the yardsticks finds the tags 0, 1, 3, 4 and nothing else, and holds the margins."""
    import corner_ref
    import detect_ref
    scale = 257 if dtype == np.uint16 else 1
    imgs, truth = tag_ref.grid_frames(dtype)
    cut_x = int(round(np.concatenate([truth[0][2][:, 0], truth[0][5][:, 0]]).mean()))
    part = np.ascontiguousarray(imgs[0][:, :cut_x])
    cand = detect_ref.detect(part, 1, 5, 1, 102, 4096)["xy"].astype(np.float64)
    r = corner_ref.refine(part, cand, tag_ref.GRID_HALF_WIN, 30, 1e-3)
    xy = ref.merge_points(np.float32(r["xy"][r["status"] == 0]).astype(np.float64))
    got = ref.propose(part, xy, max_side=max(part.shape) / 2.0, min_contrast=40.0 * scale)
    assert got["edge_margin"] >= ref.EDGE_MARGIN and got["rel_margin"] >= ref.REL_MARGIN and got["flags"] == 0
    ids = [tag_ref.decode_one(part, q, tag_ref.GRID_D, tag_ref.GRID_BORDER, tag_ref.grid_family().codes, 3, 40.0 * scale, 0, 2) for q in got["quads"]]
    assert sorted(d["id"] for d in ids) == [0, 1, 3, 4] and all(d["reason"] == tag_ref.OK for d in ids)


def test_the_merge_on_the_refined_fixture_points():
    """At nms_radius 5 no two candidates refine onto one saddle; at 3 some do (two candidates 4 px apart converge), and as separate
    points they would multiply outlines.  Merged, both sets give the six outlines."""
    imgs, _ = tag_ref.grid_frames(np.uint8)
    dropped = {}
    for nms in (5, 3):
        dropped[nms] = 0
        for k, (refined, merged) in enumerate(ref.fixture_points(np.uint8, nms)):
            assert np.array_equal(merged, api.merge_points(refined))
            d = np.abs(merged[:, None, :] - merged[None, :, :]).max(axis=2) + 2.0 * np.eye(len(merged))
            assert d.min() > 1.0
            dropped[nms] += len(refined) - len(merged)
            r = ref.propose(imgs[k], merged, **ref.fixture_params(np.uint8))
            assert (r["count"], r["flags"]) == (6, 0) and r["edge_margin"] >= 20.0
    assert dropped[5] == 0 and dropped[3] >= 4


# ---- the rule's cases ------------------------------------------------------------------------------------------------------------------
def _sheet(seed=7, strays=25):
    """tag_ref._painted_sheet (20 tags of 48 px, d = 6, one border cell) with its exact outlines and seeded stray points."""
    img, quads = tag_ref._painted_sheet(6, 1, tag_ref.small_family(6), np.uint8, 3)
    outlines = quads[0::3]
    rng = np.random.default_rng(seed)
    pts = np.concatenate([outlines.reshape(-1, 2), rng.uniform([0.0, 0.0], [319.0, 239.0], (strays, 2))])
    return img, pts, outlines


def _propose(img, pts, **kw):
    """The sheet's corners lie on a lattice of 8 px, where 120^2 is a squared distance that occurs exactly: max_side 100."""
    r = ref.propose(img, pts, **dict(dict(max_side=100.0), **kw))
    assert r["edge_margin"] >= ref.EDGE_MARGIN and r["rel_margin"] >= ref.REL_MARGIN
    return r


def test_a_painted_sheet_gives_exactly_its_outlines_in_lexicographic_order():
    img, pts, outlines = _sheet()
    r = _propose(img, pts)
    assert (r["count"], r["flags"]) == (20, 0)
    assert r["idx"].tolist() == [[4 * t, 4 * t + 1, 4 * t + 2, 4 * t + 3] for t in range(20)]
    assert np.array_equal(r["quads"], outlines)
    assert r["idx"].tolist() == sorted(r["idx"].tolist())


def test_each_outline_appears_once_whichever_corner_has_the_smallest_index():
    img, pts, outlines = _sheet()
    for seed in range(4):
        perm = np.random.default_rng(seed).permutation(len(pts))        # new index i holds the old point perm[i]
        r = _propose(img, pts[perm])
        assert r["count"] == 20 and r["idx"].tolist() == sorted(r["idx"].tolist())
        seen = set()
        for row, q in zip(r["idx"], r["quads"]):
            assert row[0] == row.min()
            old = perm[row]
            t = old[0] // 4
            assert sorted(old.tolist()) == [4 * t, 4 * t + 1, 4 * t + 2, 4 * t + 3] and ref.same_outline(q, outlines[t], 0.0)
            seen.add(int(t))
        assert seen == set(range(20))


def test_a_counter_clockwise_input_order_makes_no_difference():
    img, pts, outlines = _sheet()
    ccw = np.concatenate([outlines[:, ::-1].reshape(-1, 2), pts[80:]])
    r = _propose(img, ccw)
    assert r["count"] == 20
    for t, q in enumerate(r["quads"]):                                    # clockwise in the image all the same
        area = 0.5 * sum(q[i][0] * q[(i + 1) % 4][1] - q[(i + 1) % 4][0] * q[i][1] for i in range(4))
        assert area > 0 and ref.same_outline(q, outlines[t], 0.0)


def test_cap_below_the_count_stores_the_first_and_reports_all():
    img, pts, _ = _sheet()
    full, cut = _propose(img, pts), _propose(img, pts, cap=7)
    assert cut["count"] == 20 and len(cut["idx"]) == 7 and np.array_equal(cut["idx"], full["idx"][:7])
    assert np.array_equal(cut["quads"], full["quads"][:7])


def test_out_edge_overflow_sets_the_flag_and_collinear_chains_are_no_quads():
    case = ref.overflow_case()
    r = ref.yardstick(case)[0]
    assert r["deg"].tolist() == [11 - i for i in range(12)]
    assert (r["count"], r["flags"]) == (0, ref.FLAG_CUT)
    # the same points listed the other way round: the edges still lead towards larger x, now towards smaller indices
    back = ref.propose(case["images"][0], case["xy_list"][0][::-1], min_side=6.0)
    assert back["deg"].tolist() == [i for i in range(12)] and back["flags"] == ref.FLAG_CUT


def test_sample_points_outside_the_image_give_no_edge():
    case = ref.outside_case()
    r = ref.yardstick(case)[0]
    pts = case["xy_list"][0]
    assert r["count"] == 1 and r["idx"].tolist() == [[5, 6, 7, 8]]        # the tag well inside
    assert r["deg"][3] == 0                                              # bottom-left -> top-left of the tag at the border: outer samples at x < 0
    assert r["deg"][[0, 1, 2]].tolist() == [1, 1, 1]                     # its other three sides are edges
    assert r["deg"][4] == 0 and r["deg"][9] == 0 and not np.isfinite(pts[[4, 9]]).all()


def test_duplicate_points_duplicate_outlines_and_the_merge_removes_them():
    img, pts, outlines = _sheet(strays=0)
    dup = np.concatenate([pts, pts[[0, 5]], pts[[0]] + [0.4, -0.7]])     # corner 0 three times, corner 5 twice
    r = _propose(img, dup)
    assert r["count"] == 20 + 2 + 1
    merged = api.merge_points(dup)
    assert np.array_equal(merged, pts) and np.array_equal(merged, ref.merge_points(dup))
    assert _propose(img, merged)["count"] == 20
    # within 1 px in one coordinate only: kept
    assert len(api.merge_points([[10.0, 10.0], [10.5, 11.5], [11.0, 10.0], [12.5, 10.0]])) == 3
    assert api.merge_points(np.zeros((0, 2))).shape == (0, 2)


class _RecordingContext:
    """What api.propose_quads and api.detect_aprilgrid ask of a context, recorded: every step answers "nothing found"."""

    def __init__(self):
        self.calls = []

    def detect_corners_batch(self, images, *args):
        self.calls.append(("detect", args))
        return [(np.zeros((0, 2), np.int32), np.zeros((0, 3), np.int32), np.zeros(0, np.int64), 0) for _ in images]

    def refine_corners_batch(self, images, xy_list, *args):
        self.calls.append(("refine", args))
        n = len(images)
        return [np.zeros((0, 2))] * n, [np.zeros(0, np.int32)] * n, [np.zeros(0, np.int32)] * n, [np.zeros(0)] * n

    def propose_quads_batch(self, images, xy_list, min_side, max_side, max_side_ratio, offset, samples, min_contrast, max_per_image=1024):
        self.calls.append(("propose", dict(xy_list=xy_list, min_side=min_side, max_side=max_side, max_side_ratio=max_side_ratio,
                                           offset=offset, samples=samples, min_contrast=min_contrast, max_per_image=max_per_image)))
        return [(np.zeros((0, 4), np.int32), np.zeros((0, 4, 2)), 0, 0) for _ in images]

    def decode_tags_batch(self, images, quads_list, family_bits, codes, border, samples, min_contrast, max_border_errors, max_hamming):
        self.calls.append(("decode", dict(border=border, min_contrast=min_contrast, max_hamming=max_hamming, family_bits=family_bits)))
        n = len(images)
        return tuple([np.zeros(0, t)] * n for t in (np.int32, np.int32, np.int32, np.int32)) + \
            ([np.zeros((0, 4, 2))] * n, [np.zeros(0, np.uint64)] * n, [np.zeros(0)] * n)


def test_the_offset_follows_the_family_and_the_border():
    """offset = 1 / (2 (d + 2 border)), half a cell, whatever the family: d = 6 and 8, border 1 and 2; an explicit offset wins;
    without a family 1/16.  The points reach the context merged, and detect_aprilgrid hands its one min_contrast to both steps."""
    imgs = [np.zeros((45, 67), np.uint8)] * 2
    pts = [np.array([[5.0, 5.0], [5.5, 5.5], [30.0, 9.0]]), np.zeros((0, 2))]
    fam6 = api.TagFamily("six", 36, tag_ref.grid_family().codes)
    fam8 = api.TagFamily("eight", 64, tag_ref.small_family(8))
    for family, border, explicit, want in ((fam6, 1, None, 1.0 / 16.0), (fam6, 2, None, 1.0 / 20.0), (fam8, 1, None, 1.0 / 20.0),
                                           (fam8, 2, None, 1.0 / 24.0), (None, 1, None, 1.0 / 16.0), (fam8, 2, 0.1, 0.1)):
        rec = _RecordingContext()
        got = api.propose_quads(imgs, pts, family, border=border, offset=explicit, min_contrast=33.0, ctx=rec)
        (step, a), = rec.calls
        assert step == "propose" and a["offset"] == want and a["min_contrast"] == 33.0 and a["max_side"] is None
        assert [len(x) for x in a["xy_list"]] == [2, 0] and np.array_equal(a["xy_list"][0], pts[0][[0, 2]])
        assert [(q.shape, c, f) for q, c, f in got] == [((0, 4, 2), 0, 0)] * 2
    for family, border, want in ((fam6, 1, 1.0 / 16.0), (fam8, 2, 1.0 / 24.0)):
        rec = _RecordingContext()
        assert api.detect_aprilgrid(imgs, family, api.AprilGridBoard(), min_contrast=51.0, border=border, max_hamming=1, ctx=rec) == [None, None]
        steps = dict(rec.calls)
        assert [s for s, _ in rec.calls] == ["detect", "refine", "propose", "decode"]
        assert steps["propose"]["offset"] == want and steps["propose"]["min_contrast"] == 51.0
        assert steps["decode"] == dict(border=border, min_contrast=51.0, max_hamming=1, family_bits=family.bits)
        assert steps["refine"][0] == 4                                       # half_win: the default that suits cells of 5 to 6 px
    with pytest.raises(ValueError):
        api.propose_quads(imgs, pts[:1], fam6, ctx=_RecordingContext())


# ---- the margin condition of the GPU fixtures -----------------------------------------------------------------------------------------
def test_every_parity_fixture_keeps_its_margins():
    names, n_pts, n_quads, cut = set(), 0, 0, 0
    for case in ref.parity_cases():
        assert case["name"] not in names
        names.add(case["name"])
        ref.check_margins(case)
        for xy, r in zip(case["xy_list"], ref.yardstick(case)):
            n_pts += len(xy)
            n_quads += r["count"]
            cut += r["flags"] & ref.FLAG_CUT
    assert n_pts > 2000 and n_quads > 500 and cut >= 3
    counts = sorted({len(xy) for c in ref.sheet_cases() for xy in c["xy_list"]})
    assert counts == [0, 1, 3, 4, 63, 64, 65, 130]
    assert {c["samples"] for c in ref.sheet_cases()} == {1, 8, 16}
    shapes = {c["images"].shape[1:] for c in ref.sheet_cases()}
    assert (45, 67) in shapes and (160, 200) in shapes
