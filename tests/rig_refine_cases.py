"""The rigs and slots that tests/test_gpu_rig_refine.py runs, built without a GPU so that the yardstick's own figures on exactly
these slots (the constants at the top of that test) can be measured on a CPU: `PYTHONPATH=. python tests/rig_refine_cases.py` prints them."""
import functools

import numpy as np

from camera_intrinsic_calibration_rs_amd import synth

# two rigs of different cameras with large extrinsic rotations (0.44 and 0.43 rad)
RIGS = {
    "A": (["eucm", "kb4"], [[0.0] * 6, [0.3, -0.25, 0.2, -0.1, 0.02, 0.01]]),
    "B": (["ucm", "opencv5", "eucm"], [[0.0] * 6, [0.3, -0.25, 0.2, -0.1, 0.02, 0.01], [-0.2, 0.35, -0.15, 0.1, -0.03, 0.02]]),
}
EXACT_SEED = {"A": 2, "B": 1}         # the first seeds at which every slot is seen and every segment count occurs
NOISY_SEED = 3
# What measure() below gave for the yardstick on these slots (numpy f64, EXPERIMENTS.md): the bounds of tests/test_gpu_rig_refine.py
# are 10 x these.  exact(): yardstick against ground truth per rig; noisy(): its two-start difference and its relative gradient.
YARD_EXACT_R = {"A": 1.124e-15, "B": 8.327e-16}
YARD_EXACT_T = {"A": 2.220e-16, "B": 4.441e-16}
YARD_NOISY_R, YARD_NOISY_T = 2.380e-10, 5.777e-11
YARD_GRAD_REL = 2.179e-9


def rig_of(sp, extr=None):
    """(models, params, extr) of a synthetic rig at its ground truth."""
    models = [int(m) for m in sp.model]
    params = [sp.intr_gt[c, :synth.MODEL_NPARAMS[m]].copy() for c, m in enumerate(models)]
    return models, params, np.asarray(sp.extr_gt if extr is None else extr, dtype=np.float64)


def slots_of(sp, uv=None):
    """One list of segments (cam, X, uv) per slot, cameras in index order, f64 copies of the f32 data (uv: other detections)."""
    uv = sp.p2d.astype(np.float64) if uv is None else uv
    slots = [[] for _ in range(sp.n_slots)]
    for o in range(sp.n_obs):
        a, b = int(sp.obs_offsets[o]), int(sp.obs_offsets[o + 1])
        slots[int(sp.obs_slot[o])].append((int(sp.obs_cam[o]), sp.p3d[a:b].astype(np.float64), uv[a:b].copy()))
    return slots


def exact_uv(sp):
    """Every detection recomputed in f64 at the true T_c_0 o T_0_b."""
    uv = np.zeros((sp.n_corners, 2))
    Rc = synth.rodrigues(sp.extr_gt[:, :3])
    for o in range(sp.n_obs):
        a, b = int(sp.obs_offsets[o]), int(sp.obs_offsets[o + 1])
        c, s = int(sp.obs_cam[o]), int(sp.obs_slot[o])
        p0 = sp.p3d[a:b].astype(np.float64) @ synth.rodrigues(sp.poses_gt[s, :3]).T + sp.poses_gt[s, 3:]
        uv[a:b] = synth.project(int(sp.model[c]), sp.intr_gt[c], p0 @ Rc[c].T + sp.extr_gt[c, 3:])
    return uv


@functools.lru_cache(maxsize=None)
def exact(name):
    """12 slots of rig `name`, uv exact; the start 0.05 rad / 0.02 m off (as tests/test_gpu_refine.py builds it)."""
    models, extr = RIGS[name]
    sp = synth.make_rig(12, models, extr, seed=EXACT_SEED[name], noise_px=0)
    slots = slots_of(sp, exact_uv(sp))
    assert all(slots), "a slot that no camera sees: choose another seed"
    sgn = np.where(synth.uniform01(0xE7AC7, 12 * 6, stream=40).reshape(12, 6) < 0.5, -1.0, 1.0)
    start = sp.poses_gt + sgn * np.array([0.05, 0.05, 0.05, 0.02, 0.02, 0.02]) / np.sqrt(3.0)
    return rig_of(sp), slots, start, sp.poses_gt


@functools.lru_cache(maxsize=None)
def noisy():
    """24 slots of rig A, 0.1 px noise, 5 % of the corners displaced by 20 px in a random direction; the start is make_rig's."""
    models, extr = RIGS["A"]
    sp = synth.make_rig(24, models, extr, seed=NOISY_SEED, noise_px=0.1)
    n = sp.n_corners
    bad = synth.uniform01(0x0071E5, n, stream=31) < 0.05
    ang = 2.0 * np.pi * synth.uniform01(0x0071E5, n, stream=32)
    uv = sp.p2d.astype(np.float64)
    uv[bad] += 20.0 * np.stack([np.cos(ang), np.sin(ang)], axis=1)[bad]
    slots = slots_of(sp, uv.astype(np.float32).astype(np.float64))
    assert all(slots), "a slot that no camera sees: choose another seed"
    assert any(len(s) == 1 for s in slots) and any(len(s) == 2 for s in slots)
    return rig_of(sp), slots, sp.poses0.copy(), sp.poses_gt


@functools.lru_cache(maxsize=None)
def yardstick_noisy():
    """The yardstick on the noisy slots: computed once, shared, never changed.  Per slot (pose, cost, pose of the run from the
    start, pose of the run from the ground truth)."""
    import rig_refine_ref as ref
    rig, slots, start, gt = noisy()
    out = []
    for s, slot in enumerate(slots):
        ra = ref.refine(rig, slot, start[s], 1.0)
        rb = ref.refine(rig, slot, gt[s], 1.0)
        best = ra if ref.objective(rig, slot, ra[0], 1.0) <= ref.objective(rig, slot, rb[0], 1.0) else rb
        out.append((best[0], best[1], ra[0], rb[0]))
    return out


def dR(p, q):
    return float(np.abs(synth.rodrigues(np.asarray(p)[..., :3]) - synth.rodrigues(np.asarray(q)[..., :3])).max())


def measure():
    """The yardstick's own figures on the slots above (EXPERIMENTS.md, the constants of tests/test_gpu_rig_refine.py): printed and
    returned - exact_r / exact_t per rig, noisy_r / noisy_t / grad, and per noisy slot the two-start difference and gradient ratio."""
    import rig_refine_ref as ref
    names = {v: k for k, v in synth.MODEL_NAMES.items()}
    out = {"exact_r": {}, "exact_t": {}}
    for name in RIGS:
        rig, slots, start, gt = exact(name)
        worst = {}
        for s, slot in enumerate(slots):
            p = ref.refine(rig, slot, start[s], 1.0)[0]
            key = "+".join(names[rig[0][c]] for c, _, _ in slot)
            r, t = dR(p, gt[s]), float(np.abs(p[3:] - gt[s, 3:]).max())
            if r >= worst.get("r", (-1,))[0]: worst["r"] = (r, key, s)
            if t >= worst.get("t", (-1,))[0]: worst["t"] = (t, key, s)
        out["exact_r"][name], out["exact_t"][name] = worst["r"][0], worst["t"][0]
        print(f"exact {name}: yardstick - truth dR {worst['r'][0]:.3e} (models {worst['r'][1]}, slot {worst['r'][2]}) "
              f"dt {worst['t'][0]:.3e} (models {worst['t'][1]}, slot {worst['t'][2]})")
    rig, slots, start, gt = noisy()
    y = yardstick_noisy()
    out["slot_diff"] = [max(dR(r[2], r[3]), float(np.abs(r[2][3:] - r[3][3:]).max())) for r in y]
    out["noisy_r"] = max(dR(r[2], r[3]) for r in y); out["noisy_t"] = max(float(np.abs(r[2][3:] - r[3][3:]).max()) for r in y)
    out["slot_grad"] = []
    for s, slot in enumerate(slots):
        g0 = np.linalg.norm(ref.gradient(rig, slot, start[s], 1.0))
        out["slot_grad"].append(float(np.linalg.norm(ref.gradient(rig, slot, y[s][0], 1.0)) / g0))
    out["grad"] = max(out["slot_grad"])
    far = max(max(dR(r[2], gt[s]), float(np.abs(r[2][3:] - gt[s, 3:]).max())) for s, r in enumerate(y))
    print(f"noisy A: two-start self-difference dR {out['noisy_r']:.3e} dt {out['noisy_t']:.3e}; |grad| / |grad at the start| {out['grad']:.3e}; "
          f"segments per slot {[len(s) for s in slots]}; result - truth <= {far:.2e}")
    return out


if __name__ == "__main__":
    measure()
