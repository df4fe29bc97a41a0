"""CPU: the numpy yardstick of the general PnP (tests/pnp_ref.py) recovers ground truth on the three non-planar targets of synth.py,
make_problem's `board` argument leaves the default arrays alone, and the PnP kernel compiles for gfx950 without scratch memory."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from camera_intrinsic_calibration_rs_amd import synth

import pnp_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGETS = {"hinged": synth.hinged_boards, "offset": synth.offset_board, "cube": lambda: synth.cube_points(100)}


def test_target_shapes():
    hb = synth.hinged_boards().astype(np.float64)
    assert hb.shape == (288, 3)
    na = np.cross(hb[1] - hb[0], hb[3] - hb[0]); nb = np.cross(hb[145] - hb[144], hb[147] - hb[144])
    assert abs(na @ nb) / (np.linalg.norm(na) * np.linalg.norm(nb)) < 1e-6                    # the two grids meet at 90 degrees
    assert np.abs(hb[:144] @ na - hb[0] @ na).max() < 1e-6 and np.abs(hb[144:] @ nb - hb[144] @ nb).max() < 1e-6
    ob = synth.offset_board()
    assert ob.shape == (144, 3) and (ob[:, 2] != 0).all() and abs(float(ob[0, 2]) - 0.25) < 1e-6
    assert np.linalg.svd(ob.astype(np.float64) - ob.mean(axis=0))[1][2] < 1e-5                # coplanar up to the f32 rounding of 144 points
    cb = synth.cube_points(100)
    assert cb.shape == (100, 3) and (cb.max(axis=0) - cb.min(axis=0) <= 0.5).all()
    assert np.array_equal(cb, synth.cube_points(100)) and np.linalg.svd(cb - cb.mean(axis=0))[1][2] > 0.5


@pytest.mark.parametrize("target", sorted(TARGETS))
def test_yardstick_recovers_ground_truth(target):
    sp = synth.make_problem(20, "eucm", noise_px=0, board=TARGETS[target]())
    for f in range(20):
        a, b = sp.obs_offsets[f], sp.obs_offsets[f + 1]
        X = sp.p3d[a:b].astype(np.float64)
        xn = pnp_ref.true_normalised_points(X, sp.poses_gt[f])
        R, t, E = pnp_ref.solve(X, xn)
        # E is flat to second order at its minimum and a noise-free minimum is E = 0 up to rounding (~1e-16 of the terms): the pose is
        # determined to ~sqrt(1e-16) = 1e-8
        assert np.abs(R - synth.rodrigues(sp.poses_gt[f, :3])).max() < 1e-6, (f, np.abs(R - synth.rodrigues(sp.poses_gt[f, :3])).max())
        assert np.abs(t - sp.poses_gt[f, 3:]).max() < 1e-6
        assert E < 1e-12


def test_yardstick_omega_is_the_cost():
    """vec(R)^T Omega vec(R) with t = P vec(R) - R centroid equals E recomputed from the definition, for any rotation."""
    sp = synth.make_problem(2, "eucm", board=synth.hinged_boards())
    X = sp.p3d[:288].astype(np.float64)
    xn = pnp_ref.true_normalised_points(X, sp.poses_gt[0]) + 1e-3 * synth.normal01(5, 576).reshape(288, 2)
    Om, P, cen = pnp_ref.omega_p(X, xn)
    for rv in ([0.3, -0.2, 0.5], [2.0, 1.0, -0.4]):
        R = synth.rodrigues(np.array(rv))
        t = P @ R.reshape(9) - R @ cen
        assert abs(R.reshape(9) @ Om @ R.reshape(9) / pnp_ref.cost(X, xn, R, t) - 1) < 1e-9


def test_board_none_is_todays_problem():
    """make_problem(..., board=None) gives the arrays it gave before the argument existed (digests recorded from that version), and
    an explicit default board the same."""
    want = {
        (6, "eucm", False): "c811c3418df254cc", (5, "kb4", True): "43e09bfd4504cdb0",
    }
    for (n, model, ragged) in want:
        a = synth.make_problem(n, model, ragged=ragged)
        b = synth.make_problem(n, model, ragged=ragged, board=None)
        c = synth.make_problem(n, model, ragged=ragged, board=synth.default_board())
        for other in (b, c):
            for name in ("p3d", "p2d", "obs_offsets", "poses_gt", "poses0", "intr0", "extr0", "obs_cam", "obs_slot"):
                assert np.array_equal(getattr(a, name), getattr(other, name)), name
        assert a.p3d.dtype == np.float32 and a.p2d.dtype == np.float32
        assert _digest(a) == want[(n, model, ragged)], (n, model, ragged, _digest(a))


def _digest(sp):
    h = hashlib.sha256()
    for name in ("p3d", "p2d", "obs_offsets", "poses_gt", "poses0", "intr0"):
        h.update(np.ascontiguousarray(getattr(sp, name)).tobytes())
    return h.hexdigest()[:16]


def test_pnp_kernel_needs_no_scratch(tmp_path):
    """The compiler's resource remark for gfx950: ScratchSize 0 for every instantiation of k_pose_pnp (four camera models, the
    division model, points given directly)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    csrc = os.path.join(ROOT, "camera_intrinsic_calibration_rs_amd", "csrc")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=fast", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "ccal_kernels_pnp.hip"),
                        "-o", str(tmp_path / "pnp.out")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S*k_pose_pnp\S*)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == 6 and len(scratch) == 6, (names, scratch)
    assert scratch == [0] * 6, list(zip(names, scratch))
