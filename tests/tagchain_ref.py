"""The numpy yardstick of ccal_detect_tags_*: the links the rule in include/ccal.h adds - merge, select - restated, and chain(),
which composes the four stage yardsticks (detect_ref, corner_ref, quad_ref, tag_ref) through them.  Also the fixtures the CPU and
GPU tests of the chain share: the option sets, the montages, the mixed batch and the chunk limits."""
import functools

import numpy as np

import corner_ref
import detect_ref
import quad_ref
import tag_ref

FLAG_CUT, FLAG_CAND_CAP, FLAG_QUAD_CAP, FLAG_TAG_CAP = 1, 2, 4, 8

# the options of the Python layer's defaults for the 320 x 240 fixture of tag_ref (d = 6, one border cell), 8-bit grey levels
OPTS = dict(step=1, nms_radius=5, min_response=1, rel_q10=102, cand_cap=4096, half_win=tag_ref.GRID_HALF_WIN, max_iterations=30, eps=1e-3,
            merge_radius=1.0, min_side=20.0, max_side=160.0, max_side_ratio=2.0, offset=1.0 / 16.0, edge_samples=8, edge_min_contrast=40.0,
            quad_cap=1024, border=1, cell_samples=3, tag_min_contrast=40.0, max_border_errors=0, max_hamming=2, tag_cap=40)


def opts(dtype=np.uint8, width=tag_ref.GRID_W, height=tag_ref.GRID_H, **change):
    """OPTS for images of the given type and size (contrasts in the type's grey levels, max_side half the larger side), then `change`."""
    scale = 257.0 if np.dtype(dtype) == np.uint16 else 1.0
    return dict(dict(OPTS, max_side=max(width, height) / 2.0, edge_min_contrast=40.0 * scale, tag_min_contrast=40.0 * scale), **change)


def merge(xy, radius):
    """Step 5: the points [n, 2] in order; a point is dropped if |dx| <= radius and |dy| <= radius against a point KEPT before it."""
    pts = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    kept = np.zeros((len(pts), 2))
    n = 0
    for p in pts:
        if not (np.abs(kept[:n] - p) <= radius).all(axis=1).any():
            kept[n] = p
            n += 1
    return kept[:n].copy()


def select(reason, tag_id, hamming, margin):
    """Step 8: the rows that keep their id, in ascending id.  Among the OK rows of an id the smallest (hamming, -margin, row)."""
    best = {}
    for j in np.flatnonzero(np.asarray(reason) == tag_ref.OK):
        t, key = int(tag_id[j]), (int(hamming[j]), -float(margin[j]), int(j))
        if t not in best or key < best[t]:
            best[t] = key
    return [best[t][2] for t in sorted(best)]


def chain(img, d, codes, o):
    """One image through the rule: {"count", "id", "rot", "hamming" int32 [m], "corners" [m, 4, 2], "margin" [m], "flags", "stats",
    and, for the tests' own assertions, "refined" (the rounded points before the merge), "points", "quads", "decoded"}, m = min(count, tag_cap)."""
    det = detect_ref.detect(img, o["step"], o["nms_radius"], o["min_response"], o["rel_q10"], o["cand_cap"])
    r = corner_ref.refine(img, det["xy"].astype(np.float64), o["half_win"], o["max_iterations"], o["eps"])
    refined = np.float32(np.asarray(r["xy"]).reshape(-1, 2)[np.asarray(r["status"]).reshape(-1) == 0]).astype(np.float64)
    points = merge(refined, o["merge_radius"])
    q = quad_ref.propose(img, points, o["min_side"], o["max_side"], o["max_side_ratio"], o["offset"], o["edge_samples"],
                         o["edge_min_contrast"], o["quad_cap"])
    dec = [tag_ref.decode_one(img, quad, d, o["border"], codes, o["cell_samples"], o["tag_min_contrast"], o["max_border_errors"],
                              o["max_hamming"]) for quad in q["quads"]]
    win = select([x["reason"] for x in dec], [x["id"] for x in dec], [x["hamming"] for x in dec], [x["margin"] for x in dec])
    m = min(len(win), o["tag_cap"])
    flags = (q["flags"] & FLAG_CUT) | (FLAG_CAND_CAP if det["count"] > o["cand_cap"] else 0) | \
        (FLAG_QUAD_CAP if q["count"] > o["quad_cap"] else 0) | (FLAG_TAG_CAP if len(win) > o["tag_cap"] else 0)
    return {"count": len(win), "id": np.array([dec[j]["id"] for j in win[:m]], dtype=np.int32),
            "rot": np.array([dec[j]["rot"] for j in win[:m]], dtype=np.int32),
            "hamming": np.array([dec[j]["hamming"] for j in win[:m]], dtype=np.int32),
            "corners": np.array([dec[j]["corners"] for j in win[:m]], dtype=np.float64).reshape(m, 4, 2),
            "margin": np.array([dec[j]["margin"] for j in win[:m]], dtype=np.float64), "flags": flags,
            "stats": [det["count"], len(points), q["count"], sum(x["reason"] == tag_ref.OK for x in dec)],
            "refined": refined, "points": points, "quads": q, "decoded": dec}


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------------
MONTAGES = ((0, 2), (1, 3))


@functools.lru_cache(maxsize=None)
def montage(which, dtype=np.uint8):
    """Two frames of tag_ref.grid_frames side by side, 640 x 240: every tag id 0 .. 5 is in the image twice."""
    imgs, _ = tag_ref.grid_frames(dtype)
    a, b = MONTAGES[which]
    out = np.ascontiguousarray(np.concatenate([imgs[a], imgs[b]], axis=1))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def cropped_frame(dtype=np.uint8):
    """Frame 0 cut through the middle of its right tag column: four whole tags (the crop of tests/test_gpu_quads.py)."""
    imgs, truth = tag_ref.grid_frames(dtype)
    cut_x = int(round(np.concatenate([truth[0][2][:, 0], truth[0][5][:, 0]]).mean()))
    return np.ascontiguousarray(imgs[0][:, :cut_x])


@functools.lru_cache(maxsize=None)
def mixed_batch(dtype=np.uint8):
    """[4][240][W]: a fixture frame, an all-zero image, a plain checkerboard (points, no tags) and the cropped frame, every image
    cut to the crop's width."""
    imgs, _ = tag_ref.grid_frames(dtype)
    part = cropped_frame(dtype)
    W = part.shape[1]
    board = detect_ref.board_frames(dtype)[0][0]
    out = np.ascontiguousarray(np.stack([imgs[1][:, :W], np.zeros_like(part), board[:, :W], part]))
    out.setflags(write=False)
    return out


# ---- the planner (csrc/ccal_tagchain_plan.hpp) restated -----------------------------------------------------------------------------
PER_SLOT, PER_CAND, PER_QUAD, PER_TAG, PER_IMAGE, MAX_IMAGES = 24, 136, 180, 84, 64, 65535


def plan_model(on_device, width, height, itemsize, step, r, cand_cap, quad_cap, tag_cap, n_codes, limit, n_img):
    """(bytes per image, images per chunk): the caps cut to what the image's size allows, the rows' bytes added up."""
    d0 = step + 2
    if width <= 2 * d0 or height <= 2 * d0:
        slots = dh = cand = quads = tags = 0
    else:
        dw, dh = width - 2 * d0, height - 2 * d0
        slots = -(-dw // (r + 1)) * -(-dh // (r + 1))
        cand = min(cand_cap, slots)
        quads = min(quad_cap, 512 * cand)
        tags = min(tag_cap, quads, n_codes)
    per = (0 if on_device else itemsize * width * height) + PER_SLOT * slots + 4 * dh + PER_CAND * cand + PER_QUAD * quads + \
        PER_TAG * tags + PER_IMAGE
    return per, min(n_img, MAX_IMAGES, max(limit // per, 1))


BOARD_PER_CAND, BOARD_PER_KEPT, BOARD_PER_CORNER, BOARD_MAX_KEPT = 28 + 56, 108, 16, 512


def board_plan_model(on_device, width, height, itemsize, step, r, cand_cap, corners, limit, n_img):
    """plan_model for ccal_detect_checkerboards_*: per candidate the detector's stored row and the assembly's input row, per kept slot
    (at most 512 of the candidates) the assembly's work, 16 bytes per corner of the cols x rows = `corners` board."""
    d0 = step + 2
    if width <= 2 * d0 or height <= 2 * d0:
        slots = dh = cand = 0
    else:
        dw, dh = width - 2 * d0, height - 2 * d0
        slots = -(-dw // (r + 1)) * -(-dh // (r + 1))
        cand = min(cand_cap, slots)
    per = (0 if on_device else itemsize * width * height) + PER_SLOT * slots + 4 * dh + BOARD_PER_CAND * cand + \
        BOARD_PER_KEPT * min(cand, BOARD_MAX_KEPT) + BOARD_PER_CORNER * corners + PER_IMAGE
    return per, min(n_img, MAX_IMAGES, max(limit // per, 1))


def chunk_limit(on_device, shape, itemsize, o, n_codes, images_per_chunk):
    """A byte limit at which the planner puts exactly `images_per_chunk` images of `shape` = (H, W) into a chunk."""
    per, _ = plan_model(on_device, shape[1], shape[0], itemsize, o["step"], o["nms_radius"], o["cand_cap"], o["quad_cap"], o["tag_cap"],
                        n_codes, 0, 1)
    return per * images_per_chunk + per // 2
