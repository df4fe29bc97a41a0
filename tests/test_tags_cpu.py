"""CPU: the tag decoder's rule as tests/tag_ref.py restates it (the yardstick the GPU tests hold the kernel to), its conventions
decided by rendered tags, the board and frame layer of the api (AprilGridBoard, TagFamily, frames_from_tags), and the margin
condition of every fixture the GPU parity tests use.  No GPU, nothing outside the repository."""
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import corner_ref  # noqa: E402
import detect_ref  # noqa: E402
import tag_ref as ref  # noqa: E402

from camera_intrinsic_calibration_rs_amd import _ffi, api  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
assert (_ffi.TAG_OK, _ffi.TAG_OUTSIDE, _ffi.TAG_LOW_CONTRAST, _ffi.TAG_BORDER, _ffi.TAG_NO_CODE) == (ref.OK, ref.OUTSIDE, ref.LOW_CONTRAST,
                                                                                                    ref.BORDER, ref.NO_CODE)


def test_reason_codes_are_the_headers():
    src = open(os.path.join(ROOT, "include", "ccal.h")).read()
    body = re.search(r"typedef enum \{([^}]*)\} ccal_tag_reason;", src, flags=re.S).group(1)
    got = {k: int(v) for k, v in re.findall(r"CCAL_TAG_([A-Z_]+)\s*=\s*(\d+)", body)}
    assert got == {name: i for i, name in enumerate(ref.REASONS)}


# ---- the map ------------------------------------------------------------------------------------------------------------------------
def test_map_sends_the_unit_squares_corners_to_the_quads():
    quad = np.array([[31.25, 17.5], [92.0, 23.75], [85.5, 88.0], [12.0, 71.25]])          # skewed: no two sides parallel
    coef = ref.quad_map(quad)
    assert abs(coef[6]) > 1e-3 and abs(coef[7]) > 1e-3                                      # g, h: a projective map, not an affine one
    for (u, v), want in zip(((0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)), quad):
        x, y, w = ref.map_point(coef, u, v)
        assert w > 0 and abs(x - want[0]) <= 1e-12 and abs(y - want[1]) <= 1e-12
    # the centre of the square goes to the crossing of the diagonals (what makes the map projective rather than bilinear)
    x, y, _ = ref.map_point(coef, 0.5, 0.5)
    A = np.array([quad[2] - quad[0], -(quad[3] - quad[1])]).T
    s = np.linalg.solve(A, quad[1] - quad[0])[0]
    assert np.allclose([x, y], quad[0] + s * (quad[2] - quad[0]), atol=1e-10)


# ---- the turn convention, decided by rendering ---------------------------------------------------------------------------------------
ONE = ref.Board(0.03, 0.3, 1, 1)


def _one_tag(code, rot_deg, dtype=np.uint8, d=6, border=1):
    cam = detect_ref.Camera(600.0, 79.5, 59.5, -0.2)
    R, t = ref.grid_pose(ONE, rot_deg, 12.0, 40.0, (0.001, -0.002, 0.25))
    img = ref.render_aprilgrid(160, 120, cam, R, t, ONE, ref.Family(d * d, (code,)), border, dtype)
    return img, ref.true_quads(cam, R, t, ONE)[0]


def test_turn_convention_against_a_rendered_tag():
    """The tag rendered at four in-plane turns.  The quad handed to the decoder starts at the corner nearest the image's top-left
    and goes round clockwise in the image, as a quad proposer would give it: it is the tag's canonical outline (the projected
    printed corners top-left, top-right, bottom-right, bottom-left) cyclically shifted by some s.  The decoder must say rot = s
    and return the canonical outline, corners_out[i] = q[(i + 3 rot) mod 4]: the sentence of the header."""
    fam = ref.make_family(6, 40, 10, 2)
    seen = set()
    for rot_deg in (5.0, 95.0, 185.0, 275.0):
        img, canon = _one_tag(fam[7], rot_deg)
        s = int(np.argmin(canon[:, 0] + canon[:, 1]))
        quad = np.roll(canon, -s, axis=0)                       # quad[i] = canon[(i + s) % 4]
        area = 0.5 * sum(quad[i][0] * quad[(i + 1) % 4][1] - quad[(i + 1) % 4][0] * quad[i][1] for i in range(4))
        assert area > 0, "clockwise in the image (y down)"
        r = ref.decode_one(img, quad, 6, 1, fam, 3, 20.0, 0, 2)
        assert (r["reason"], r["id"], r["hamming"]) == (ref.OK, 7, 0)
        assert r["rot"] == s, (rot_deg, r["rot"], s)
        assert np.array_equal(r["corners"], canon)
        assert np.array_equal(r["corners"], np.array([quad[(i + 3 * r["rot"]) % 4] for i in range(4)]))
        assert r["code"] == ref.turn_code(fam[7], 6, -s % 4)    # as read from q0: s clockwise turns of it give the code back
        assert r["margin"] >= 20.0
        seen.add(s)
    assert seen == {0, 1, 2, 3}


def test_painted_tags_follow_the_same_convention():
    """paint_tag(turns = k) - the fixture of the parity tests - decodes with rot = k from the shown top-left."""
    fam = ref.small_family(6)
    for k in range(4):
        img = np.full((64, 64), 215, dtype=np.uint8)
        q = ref.paint_tag(img, 8, 8, 6, fam[1], 6, 1, 40, 215, turns=k)
        r = ref.decode_one(img, q, 6, 1, fam, 3, 20.0, 0, 0)
        assert (r["reason"], r["id"], r["rot"], r["hamming"], r["margin"]) == (ref.OK, 1, k, 0, 87.5)


# ---- bit flips ----------------------------------------------------------------------------------------------------------------------
def test_bit_flips_up_to_max_hamming_decode_and_one_more_does_not():
    fam = ref.make_family(6, 40, 10, 2)
    for m in range(4):                                          # the family's distance, over every turn and the codes' own turns
        for k in range(4):
            for m2 in range(40):
                if (m2, k) != (m, 0):
                    assert ref.popcount(fam[m] ^ ref.turn_code(fam[m2], 6, k)) >= 10
    rng = np.random.default_rng(8)
    for flips in range(6):
        m = 11 + flips
        mask = sum(1 << int(b) for b in rng.choice(36, flips, replace=False))
        img, canon = _one_tag(fam[m] ^ mask, 20.0 + 90.0 * flips)
        r = ref.decode_one(img, canon, 6, 1, fam, 3, 20.0, 0, 4)
        if flips <= 4:
            assert (r["reason"], r["id"], r["rot"], r["hamming"]) == (ref.OK, m, 0, flips), flips
        else:
            assert (r["reason"], r["id"], r["rot"], r["hamming"]) == (ref.NO_CODE, -1, -1, -1)
            assert r["code"] == fam[m] ^ mask and np.isnan(r["corners"]).all()


# ---- ties, reasons ---------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_smaller_index_and_the_smaller_turn():
    for case in ref.tie_cases():
        r = ref.yardstick(case)[0][0]
        assert (r["reason"], r["id"], r["rot"], r["hamming"]) == (ref.OK,) + case["want"], case["name"]


def test_every_reason_has_a_case_built_for_it():
    got = {}
    for case in [ref.bounds_case()] + ref.threshold_cases():
        rs = [r["reason"] for r in ref.yardstick(case)[0]]
        assert rs == case["want_reasons"], case["name"]
        for q, r in zip(case["quads_list"][0], ref.yardstick(case)[0]):
            got.setdefault(r["reason"], []).append(r)
            if r["reason"] == ref.OUTSIDE:
                assert np.isnan(r["margin"]) and r["code"] == 0 and r["id"] == -1 and np.isnan(r["corners"]).all()
            if r["reason"] == ref.LOW_CONTRAST:
                assert r["code"] == 0 and r["margin"] == 10.5
            if r["reason"] == ref.BORDER:
                assert r["code"] == ref.small_family(6)[4] and r["id"] == -1
    for case in ref.table_cases():
        rs = ref.yardstick(case)[0]
        assert [(r["reason"], r["id"], r["hamming"]) for r in rs[:3]] == [(ref.OK, m, 1) for m in case["want"]], case["name"]
        assert [r["rot"] for r in rs[:3]] == [1, 2, 3]
        assert rs[3]["reason"] == ref.NO_CODE
        got.setdefault(ref.NO_CODE, []).append(rs[3])
    assert sorted(got) == [ref.OK, ref.OUTSIDE, ref.LOW_CONTRAST, ref.BORDER, ref.NO_CODE]
    deg = ref.degenerate_case()
    rs = ref.yardstick(deg)[0]
    assert all(rs[i]["reason"] == ref.OUTSIDE for i in deg["must_be_outside"]) and rs[0]["reason"] == ref.OK


# ---- the margin condition of the GPU fixtures -----------------------------------------------------------------------------------------
def test_every_parity_fixture_keeps_its_margin():
    """Every quad of every case the GPU parity tests run is OUTSIDE or has a yardstick margin of at least 0.5 grey levels: no cell
    sits near its threshold, so no white / black decision rides on the last bits of a sum."""
    names = set()
    n = 0
    for case in ref.parity_cases():
        assert case["name"] not in names
        names.add(case["name"])
        for per_image in ref.yardstick(case):
            for r in per_image:
                n += 1
                assert r["reason"] == ref.OUTSIDE or r["margin"] >= ref.MARGIN_FLOOR, (case["name"], ref.REASONS[r["reason"]], r["margin"])
    assert n > 1000


def e2e_quads(dtype, shift=0):
    """The end-to-end quads as the CPU pipeline gives them: the true outlines moved onto the saddles by corner_ref.refine (what
    api.refine_corners computes on the GPU, to 1e-9 px), each quad cyclically shifted by `shift`."""
    imgs, quads = ref.grid_frames(dtype)
    out = []
    for k in range(len(imgs)):
        r = corner_ref.refine(imgs[k], quads[k].reshape(-1, 2), ref.GRID_HALF_WIN, 30, 1e-3)
        assert (r["status"] == 0).all()
        out.append(np.roll(np.float32(r["xy"]).astype(np.float64).reshape(-1, 4, 2), -shift, axis=1))
    return imgs, quads, out


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_the_end_to_end_fixture_on_the_cpu(dtype):
    """The GPU end-to-end test's frames through the yardstick: all six tags of every frame, rot = the shift, Hamming distance 0,
    the refined corners within 0.2 px of the truth, and the margin condition."""
    scale = 257 if dtype == np.uint16 else 1
    for shift in (0, 1):
        imgs, truth, quads = e2e_quads(dtype, shift)
        for k in range(len(imgs)):
            for m, q in enumerate(quads[k]):
                r = ref.decode_one(imgs[k], q, ref.GRID_D, ref.GRID_BORDER, ref.grid_family().codes, 3, 20.0 * scale, 0, 2)
                assert (r["reason"], r["id"], r["rot"], r["hamming"]) == (ref.OK, m, shift, 0), (k, m, shift)
                assert r["margin"] >= ref.MARGIN_FLOOR
                assert np.linalg.norm(r["corners"] - truth[k][m], axis=1).max() <= 0.2


# ---- AprilGridBoard, TagFamily ---------------------------------------------------------------------------------------------------------
def test_aprilgrid_board_is_the_references_default_board():
    f32 = np.float32
    b = api.AprilGridBoard()
    s = f32(0.088)
    assert len(b.id_to_3d) == 144 and sorted(b.id_to_3d) == list(range(144))
    assert b.id_to_3d[0] == (0.0, 0.0, 0.0)
    assert b.id_to_3d[1] == (float(s), 0.0, 0.0)
    assert b.id_to_3d[2] == (float(s), float(-s), 0.0)
    assert b.id_to_3d[3] == (0.0, float(-s), 0.0)
    y1 = -f32(0.088) * f32(1.3)
    assert b.id_to_3d[24] == (0.0, float(y1), 0.0)                           # tag (r = 1, c = 0)
    assert b.id_to_3d[26] == (float(f32(0.0) + s), float(y1 - s), 0.0)
    x5 = f32(5.0) * s * (f32(1.0) + f32(0.3))
    assert b.id_to_3d[4 * 5 + 1] == (float(x5 + s), 0.0, 0.0)
    assert all(float(f32(v)) == v for p in b.id_to_3d.values() for v in p)  # every coordinate is an f32 number


def test_aprilgrid_board_first_id_and_json():
    b = api.AprilGridBoard(first_id=3, tag_rows=2, tag_cols=2)
    assert sorted(b.id_to_3d) == list(range(12, 28)) and b.id_to_3d[12] == (0.0, 0.0, 0.0)
    j = api.AprilGridBoard.from_json_obj(json.loads('{"tag_size_meter": 0.05, "tag_spacing": 0.25, "tag_rows": 3, "tag_cols": 4, "first_id": 2}'))
    assert (j.tag_size_meter, j.tag_spacing, j.tag_rows, j.tag_cols, j.first_id) == (0.05, 0.25, 3, 4, 2)
    assert sorted(j.id_to_3d) == list(range(8, 8 + 48))
    assert j.id_to_3d[8 + 4 * 5 + 2] == (float(np.float32(1.0) * np.float32(0.05) * (np.float32(1.0) + np.float32(0.25)) + np.float32(0.05)),
                                         float(-np.float32(1.0) * np.float32(0.05) * (np.float32(1.0) + np.float32(0.25)) - np.float32(0.05)), 0.0)
    with pytest.raises(KeyError):
        api.AprilGridBoard.from_json_obj({"tag_size": 0.05})


def test_tag_family_is_data():
    fam = api.TagFamily("toy", 36, ref.make_family(6, 40, 10, 2))
    assert fam.d == 6 and len(fam.codes) == 40
    again = api.TagFamily.from_json_obj(json.loads(json.dumps(fam.to_json_obj())))
    assert again == fam and sorted(fam.to_json_obj()) == ["bits", "codes", "name"]
    top = api.TagFamily("full", 64, [2 ** 64 - 1, 0])
    assert top.codes == (2 ** 64 - 1, 0)
    for bits in (4, 8, 35, 81, 0, -9):
        with pytest.raises(ValueError):
            api.TagFamily("bad", bits, [1])
    with pytest.raises(ValueError):
        api.TagFamily("bad", 9, [512])
    with pytest.raises(ValueError):
        api.TagFamily("bad", 9, [])


# ---- frames_from_tags ------------------------------------------------------------------------------------------------------------------
def test_frames_from_tags_mirrors_the_references_front_end():
    board = api.AprilGridBoard(0.03, 0.3, 2, 3)
    quads = np.arange(6 * 8, dtype=np.float64).reshape(6, 4, 2) + 0.1234567891
    decoded = [[(m, 0, 0, quads[m]) for m in range(6)],                       # 24 corners
               [(m, 0, 0, quads[m]) for m in range(5)] + [(9, 0, 0, quads[5])],  # tag 9 is not on the board: 20 corners
               []]
    frames = api.frames_from_tags(decoded, board, (320, 240), times=[5, 6, 7])
    assert frames[1] is None and frames[2] is None
    f = frames[0]
    assert f.time_ns == 5 and f.img_w_h == (320, 240) and sorted(f.features) == list(range(24))
    for m in range(6):
        for i in range(4):
            ft = f.features[4 * m + i]
            assert ft.p3d == board.id_to_3d[4 * m + i]
            assert ft.p2d == (float(np.float32(quads[m, i, 0])), float(np.float32(quads[m, i, 1])))
    # 23 known corners: None; the reference's MIN_CORNERS is 24
    del board.id_to_3d[13]
    assert api.frames_from_tags(decoded[:1], board, (320, 240)) == [None]
    got = api.frames_from_tags(decoded[:1], board, (320, 240), min_corners=23)[0]
    assert got.time_ns == 0 and sorted(got.features) == [i for i in range(24) if i != 13]
    # unknown ids are dropped, the rest stays
    low = api.frames_from_tags(decoded[1:2], api.AprilGridBoard(0.03, 0.3, 2, 3), (320, 240), min_corners=20)[0]
    assert sorted(low.features) == list(range(20))
    with pytest.raises(ValueError):
        api.frames_from_tags(decoded, board, (320, 240), times=[1])
