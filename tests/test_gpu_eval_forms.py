"""GPU: the two forms of the mode-E kernel - k_eval (a wavefront per frame, its passes one after another) and k_eval_fw (a
workgroup per frame, a wavefront per pass; ccal_kernels_eval.hip) - compute the same bits.

Each form runs in a child process of its own (the switch CCAL_EVAL_FORM=frame|pass of the second library is read once per
process), a third child runs the product library's automatic choice (every problem here is far below its frame limit: the
product's k_eval_fw).  A child evaluates every problem of _problems() with ccal_eval_dev into buffers that carry a guard band
of a NaN pattern in front of and behind the 2 n_corners / j_len doubles, and writes the whole buffers to a file.  The tests
then hold, per problem: frame == pass == automatic bit for bit, the oracle at test_gpu_eval's tolerances, untouched guards.

The selection rule itself (eval_frame_form) is constexpr host logic without an entry point or a test hook that reports the
form that ran; static_asserts next to it in ccal_kernels_eval.hip pin it at compile time."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)                            # (the child process runs this file as a script)

from camera_intrinsic_calibration_rs_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 512                                             # doubles in front of and behind each output
PATTERN = 0x7FF8C0DEC0DE0BAD                            # a quiet NaN no computation produces
# one pass short, exact, one over; two passes and one over; the board; three passes (one per wavefront of k_eval_fw) and one
# over (the stride loop's second round); 300 (tests/test_gpu_eval.py's largest); an EMPTY last frame
COUNTS = [1, 16, 63, 64, 65, 128, 129, 144, 192, 193, 300, 0]
OCV5_ORDER = [0, 1, 3, 4, 2]                            # k1, k2 stay; p1 -> slot 3, p2 -> slot 4, k3 -> slot 2
VARIANTS = [(m, of, c) for m in ("ucm", "eucm", "kb4", "opencv5") for of in (False, True) for c in (1, 2)]
NAMES = [f"{m}-{'one' if of else 'two'}focal-{c}cam" for m, of, c in VARIANTS] + ["eucm-single-frame-144", "opencv5-caller-order"]


def _recut(sp, counts, seed):
    """The synthetic problem with counts[slot] corners in every observation frame of that slot (drawn from the frame's own 144
    rows, with repetition beyond 144)."""
    rng = np.random.default_rng(seed)
    idx, offs = [], [0]
    for o in range(sp.n_obs):
        n = counts[int(sp.obs_slot[o])]
        a, b = int(sp.obs_offsets[o]), int(sp.obs_offsets[o + 1])
        idx.append(rng.choice(np.arange(a, b), size=n, replace=n > b - a))
        offs.append(offs[-1] + n)
    idx = np.concatenate(idx).astype(np.int64)
    return dataclasses.replace(sp, obs_offsets=np.array(offs, dtype=np.int64), p3d=sp.p3d[idx].copy(), p2d=sp.p2d[idx].copy())


def _problems():
    """name -> (problem, OPENCV5 coefficient order or None)."""
    out = {}
    for name, (model, one_focal, n_cams) in zip(NAMES, VARIANTS):
        sp = synth.make_problem(len(COUNTS), model, n_cams=n_cams, xy_same_focal=one_focal, outlier_frac=0.02, seed=0xF0F0 + n_cams)
        out[name] = (_recut(sp, COUNTS, 11), None)
    out["eucm-single-frame-144"] = (synth.make_problem(1, "eucm", outlier_frac=0.02, seed=0xF0F3), None)
    out["opencv5-caller-order"] = (_recut(synth.make_problem(len(COUNTS), "opencv5", outlier_frac=0.02, seed=0xF0F4), COUNTS, 12), OCV5_ORDER)
    return out


def _to_caller(v, order):
    """canonical OPENCV5 parameter vectors -> the caller's coefficient order"""
    out = np.array(v, dtype=np.float64, copy=True)
    for i, at in enumerate(order):
        out[..., 4 + at] = np.asarray(v)[..., 4 + i]
    return out


def _child(form, out_path):
    """Runs in the child process: every problem, both loss settings, whole guarded buffers -> out_path (.npz)."""
    import torch
    from camera_intrinsic_calibration_rs_amd import _ffi
    from camera_intrinsic_calibration_rs_amd.engine import Context, Problem
    lib = _ffi.load() if form == "auto" else _ffi.load_legacy()
    dev = torch.device("cuda", 0)
    res = {}
    for name, (sp, order) in _problems().items():
        ctx = Context(0, lib=lib)
        intr = sp.intr0
        if order is not None:
            cv = ctx.model_conventions()
            for i in range(5):
                cv.ocv5_order[i] = order[i]
            ctx.set_model_conventions(cv)
            intr = _to_caller(sp.intr0, order)
        gp = Problem.from_synth(ctx, sp)
        gp.upload_params(intr, sp.poses0, sp.extr0)
        for loss in (0, 1):
            r = torch.full((2 * gp.n_corners + 2 * GUARD,), PATTERN, dtype=torch.int64, device=dev)
            J = torch.full((gp.j_len + 2 * GUARD,), PATTERN, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            gp.eval_dev(r.data_ptr() + 8 * GUARD, J.data_ptr() + 8 * GUARD, apply_loss=bool(loss))
            ctx.sync()
            res[f"{name}/r{loss}"] = r.cpu().numpy()
            res[f"{name}/J{loss}"] = J.cpu().numpy()
        gp.close()
        ctx.close()
    np.savez(out_path, **res)
    print("FORMS-OK")


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    """form -> the arrays its child wrote (each child: a fresh process, its form set before the library loads)."""
    d = tmp_path_factory.mktemp("eval_forms")
    out = {}
    for form in ("frame", "pass", "auto"):
        env = {k: v for k, v in os.environ.items() if k != "CCAL_EVAL_FORM"}
        if form != "auto":
            env["CCAL_EVAL_FORM"] = form
        path = str(d / f"{form}.npz")
        run = subprocess.run([sys.executable, os.path.abspath(__file__), form, path], env=env, capture_output=True, text=True, timeout=600)
        assert "FORMS-OK" in run.stdout, (form, run.stdout[-2000:] + run.stderr[-4000:])
        out[form] = np.load(path)                       # read per array, when a test asks for it: nothing large stays in this process
    yield out
    for f in out.values():
        f.close()


@pytest.fixture(scope="module")
def problems():
    return _problems()


@pytest.mark.parametrize("name", NAMES)
def test_forms_agree_bit_for_bit_and_with_the_oracle(forms, problems, oracle, name):
    import test_gpu_eval as TE
    sp, order = problems[name]
    n2 = 2 * sp.n_corners
    op = oracle.OracleProblem.from_synth(sp)
    pat = np.int64(PATTERN)
    for loss in (0, 1):
        rf, Jf = forms["frame"][f"{name}/r{loss}"], forms["frame"][f"{name}/J{loss}"]
        j_len = Jf.size - 2 * GUARD
        assert rf.size == n2 + 2 * GUARD and j_len == op.j_len
        for other in ("pass", "auto"):
            assert rf.tobytes() == forms[other][f"{name}/r{loss}"].tobytes(), (name, loss, other, "r")
            assert Jf.tobytes() == forms[other][f"{name}/J{loss}"].tobytes(), (name, loss, other, "J")
        # the guard bands: not a byte in front of or behind the outputs changed (the three buffers are equal: one check)
        assert (rf[:GUARD] == pat).all() and (rf[GUARD + n2:] == pat).all(), (name, loss, "r guard")
        assert (Jf[:GUARD] == pat).all() and (Jf[GUARD + j_len:] == pat).all(), (name, loss, "J guard")
        r = rf[GUARD:GUARD + n2].view(np.float64).reshape(-1, 2)
        J = Jf[GUARD:GUARD + j_len].view(np.float64)
        ro, Jo = op.eval(sp.intr0, sp.poses0, sp.extr0, apply_loss=bool(loss))
        if order is not None:                           # the block's columns follow the caller's coefficient order
            D = 15
            cols = np.arange(D)
            for i, at in enumerate(order):
                cols[4 + at] = 4 + i
            Jo = Jo.reshape(-1, D)[:, cols].ravel()
        TE._cmp(r, J, ro, Jo)


def test_the_problems_are_the_sizes_asked_for(problems):
    assert list(problems) == NAMES
    sp = problems["eucm-twofocal-2cam"][0]
    n = np.diff(sp.obs_offsets)
    assert list(n[::2]) == COUNTS and list(n[1::2]) == COUNTS and n[-1] == 0 and sp.n_corners == 2 * sum(COUNTS)
    assert problems["eucm-single-frame-144"][0].n_corners == 144


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
