"""The frames that tests/test_gpu_pose_init.py runs through k_pose_init, built without a GPU so that tests/test_pose_init_cpu.py can
check them - and the yardstick tests/pose_init_ref.py on them - on a CPU.  `PYTHONPATH=. python tests/pose_init_cases.py` prints
what sized the constants: the worst err / (kappa^2 u) of the f64 emulation against the yardstick and the table of pivots.

A frame is a dict: name, model, params (the camera's), X [n, 3] and uv [n, 2] float32 as the library receives them, R, t (the pose
that generated it), invalid (indices of the corners moved out of the model's domain on purpose)."""
import functools

import numpy as np

from camera_intrinsic_calibration_rs_amd import synth

import pose_init_ref as ref

UCM, EUCM, KB4, OPENCV5, DIVISION = ref.UCM, ref.EUCM, ref.KB4, ref.OPENCV5, ref.DIVISION
W = H = 512.0
PARAMS = {
    UCM: np.array(synth.GT_PARAMS[UCM]), EUCM: np.array(synth.GT_PARAMS[EUCM]), KB4: np.array(synth.GT_PARAMS[KB4]),
    # mild enough that the kernel's 25 fixed-point steps reach the inverse on every corner used here (test_pose_init_cpu.py)
    OPENCV5: np.array([380.0, 380.0, 255.0, 257.0, -0.1, 0.02, 5e-4, -3e-4, -0.003]),
}
DIVISION_LAMBDA = -0.2
PARAMS[DIVISION] = ref.division_theta(W, H, DIVISION_LAMBDA)
DIST = {UCM: 0.8, EUCM: 0.8, KB4: 0.8, OPENCV5: 1.6, DIVISION: 1.2}      # board centre to camera, metres
MODEL_NAME = {UCM: "ucm", EUCM: "eucm", KB4: "kb4", OPENCV5: "opencv5", DIVISION: "division"}
COUNTS = [10, 11, 63, 64, 65, 127, 128, 129, 144, 256, 257]
RX = np.diag([1.0, -1.0, -1.0])                                            # pi about x: the board faces the camera
SEED = 0x905E1217
# The tolerance factor of tests/test_gpu_pose_init.py: 4 x the worst err / (kappa^2 u) of emulate_f64 against solve over the case list
# (0.69, measure() below), rounded up to a power of two.  tests/test_pose_init_cpu.py holds it to that rule.
F = 4.0


def board12():
    return synth.default_board()


def board18():
    """9 x 9 tags, 324 corners: the counts above 144."""
    return synth.aprilgrid_board(0.088, 0.3, 9, 9)


def _centre(board):
    return np.array([0.5 * board[:, 0].astype(np.float64).max(), 0.5 * board[:, 1].astype(np.float64).min(), 0.0])


def project(model, params, pc):
    """Pixels of camera-frame points (f64; data generation)."""
    if model != DIVISION:
        return synth.project(model, params, pc)
    xn, yn = pc[:, 0] / pc[:, 2], pc[:, 1] / pc[:, 2]
    s = 2.0 / (1.0 + np.sqrt(1.0 - 4.0 * params[4] * (xn * xn + yn * yn)))   # m = xn s with s = 1 + lambda |m|^2
    return np.stack([params[0] * xn * s + params[2], params[1] * yn * s + params[3]], axis=1)


def domain_r2_limit(model, params):
    """The squared image-plane radius |(uv - c) / f|^2 at which unproject_normalized stops returning a ray (None: no such radius)."""
    p = np.asarray(params, dtype=np.float64)
    if model == DIVISION:
        return (1.0 - 1e-9) / -p[4] if p[4] < 0 else None
    if model in (UCM, EUCM):
        alpha, beta = p[4], (p[5] if model == EUCM else 1.0)
        if alpha <= 0.5:
            return None
        hi = 1.0 / (beta * (2.0 * alpha - 1.0))
        k = lambda r2: (1.0 - alpha * alpha * beta * r2) / (alpha * np.sqrt(max(1.0 - (2.0 * alpha - 1.0) * beta * r2, 0.0)) + 1.0 - alpha)
        lo = 0.0                                                # k falls from 1 through 1e-3 before the square root ends
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if k(mid) > 1e-3 else (lo, mid)
        return lo
    if model == KB4:
        t = 1.5
        return (t * (1.0 + t * t * (p[4] + t * t * (p[5] + t * t * (p[6] + t * t * p[7]))))) ** 2
    return None


def frame(name, model, board, idx, R, t, noise_px=0.0, noise_seed=0, invalid=(), params=None):
    """The corners board[idx] seen from the pose (R, t): detections exact to f32 rounding, plus noise_px of seeded Gaussian noise;
    the corners listed in `invalid` (positions in idx) are moved to 1.5 x the radius at which the model's domain ends (r^2 = 2.25 x)."""
    params = PARAMS[model] if params is None else params
    X = np.ascontiguousarray(np.asarray(board, dtype=np.float32)[np.asarray(idx)])
    pc = X.astype(np.float64) @ R.T + t
    assert (pc[:, 2] > 0.05).all(), name
    uv = project(model, params, pc)
    if noise_px:
        uv = uv + noise_px * synth.normal01(SEED + noise_seed, 2 * len(uv), stream=4).reshape(-1, 2)
    if len(invalid):
        lim = domain_r2_limit(model, params)
        ang = 0.7 + 1.1 * np.arange(len(invalid))
        m = 1.5 * np.sqrt(lim) * np.stack([np.cos(ang), np.sin(ang)], axis=1)
        uv[list(invalid)] = m * params[:2] + params[2:4]
    return dict(name=name, model=model, params=params, X=X, uv=uv.astype(np.float32), R=R, t=t, invalid=tuple(invalid))


def look_at(R, board, dist, off=(0.0, 0.0)):
    """t that puts the board's centre at (off x dist, dist) in the camera frame."""
    return np.array([off[0] * dist, off[1] * dist, dist]) - R @ _centre(board)


def tilted(k, n):
    """n seeded rotations: the board facing the camera, then 0.1 .. 0.5 rad about a random axis."""
    u = synth.uniform01(SEED + k, 4 * n, stream=1).reshape(n, 4)
    zc = 2.0 * u[:, 0] - 1.0
    s = np.sqrt(1.0 - zc * zc)
    axis = np.stack([s * np.cos(2 * np.pi * u[:, 1]), s * np.sin(2 * np.pi * u[:, 1]), zc], axis=1)
    return synth.rodrigues(axis * (0.1 + 0.4 * u[:, 2:3])) @ RX, 0.2 * (u[:, 3] - 0.5)


def subset(board, n, k):
    """n corners of the board in a seeded random order (like the reference's HashMap iteration)."""
    return np.argsort(synth.uniform01(SEED + 31 * k, len(board), stream=3))[:n]


# ---- 1. lane and loop edges: 13 frames per model ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lane_frames(model):
    counts = COUNTS + [144, 144]                                 # 13 frames: three full workgroups and one wavefront
    Rs, offs = tilted(100 + model, len(counts))
    out = []
    for k, n in enumerate(counts):
        board = board12() if n <= 144 else board18()
        dist = DIST[model] * (1.0 if n <= 144 else 1.5)
        out.append(frame(f"{MODEL_NAME[model]}-n{n}-{k}", model, board, subset(board, n, k), Rs[k], look_at(Rs[k], board, dist, (offs[k], -offs[k]))))
    return out


# ---- 2. every rotation branch --------------------------------------------------------------------------------------------------------
ROTATIONS = [("zero", np.zeros(3)), ("1e-9", 1e-9 * np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)),
             ("2pi/3-111", 2.0 * np.pi / 3.0 * np.ones(3) / np.sqrt(3.0))]
for _name, _axis in (("x", [1.0, 0, 0]), ("y", [0, 1.0, 0]), ("z", [0, 0, 1.0]), ("xy", [np.sqrt(0.5), np.sqrt(0.5), 0])):
    ROTATIONS.append((f"pi-{_name}", (np.pi - 1e-3) * np.array(_axis)))
    ROTATIONS.append((f"pi-minus-{_name}", -(np.pi - 1e-3) * np.array(_axis)))     # the same branch with qw < 0


@functools.lru_cache(maxsize=None)
def rotation_frames():
    board = board12()
    out = []
    for name, rvec in ROTATIONS:
        R = np.eye(3) if name == "zero" else synth.rodrigues(rvec)
        off = (0.4, 0.0) if name == "2pi/3-111" else (0.05, -0.03)       # the cyclic permutation would show the board edge-on
        out.append(frame(f"rot-{name}", EUCM, board, np.arange(144), R, look_at(R, board, DIST[EUCM], off)))
    return out


# ---- 3. the count of valid corners ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def count_frames(model):
    """EUCM (alpha > 0.5) or the division model (lambda < 0).  Frames of 12 corners with 3 outside the domain (9 valid: no pose at
    min_points 10) and of 13 with 3 outside (a pose from exactly the 10 valid ones), the invalid corners first, spread and last; a
    frame of 12 or 13 corners has no lane 63, so three frames of 130 corners carry their invalid corners at 0, at 63 and at 64 and
    127 and 128 (lane 63, then lane 0 of the loop's second and third trip); and, last, a frame of 4 corners (exactly determined)."""
    board = board12()
    Rs, offs = tilted(300 + (model % 7), 9)
    spec = [(12, (0, 1, 2)), (12, (0, 5, 11)), (12, (9, 10, 11)), (13, (0, 1, 2)), (13, (0, 6, 12)), (13, (10, 11, 12)),
            (130, (0,)), (130, (63,)), (130, (64, 127, 128))]
    out = []
    for k, (n, bad) in enumerate(spec):
        out.append(frame(f"{MODEL_NAME[model]}-count{n}-bad{'_'.join(map(str, bad))}", model, board, subset(board, n, 40 + k), Rs[k],
                         look_at(Rs[k], board, DIST[model], (offs[k], offs[k])), invalid=bad))
    four = np.array([0, 46, 101, 143])                          # no three of them on a line
    out.append(frame(f"{MODEL_NAME[model]}-four", model, board, four, Rs[0], look_at(Rs[0], board, DIST[model])))
    return out


# ---- 4. conditioning -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conditioning_frames():
    board = board12()
    R = tilted(400, 1)[0][0]
    t = look_at(R, board, DIST[EUCM], (0.05, 0.02))
    all144 = np.arange(144)
    out = [frame("metres", EUCM, board, all144, R, t)]
    out.append(frame("millimetres", EUCM, (board.astype(np.float64) * 1000.0).astype(np.float32), all144, R, t * 1000.0))
    for s in (10.0, 100.0):
        shift = np.array([s, -0.7 * s, 0.0])
        out.append(frame(f"origin-{int(s)}m", EUCM, (board.astype(np.float64) + shift).astype(np.float32), all144, R, t - R @ shift))
    Rt = synth.rodrigues(np.array([0.0, np.deg2rad(75.0), 0.0])) @ RX
    out.append(frame("tilt75-5m", EUCM, board, all144, Rt, look_at(Rt, board, 5.0)))
    return out


# ---- 5. noise ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def noisy_frames():
    board = board12()
    out = []
    for model in (UCM, EUCM, KB4, OPENCV5):
        Rs, offs = tilted(500 + model, 3)
        for k, n in enumerate((144, 100, 37)):
            out.append(frame(f"noisy-{MODEL_NAME[model]}-n{n}", model, board, subset(board, n, 60 + k), Rs[k],
                             look_at(Rs[k], board, DIST[model], (offs[k], 0.0)), noise_px=0.1, noise_seed=10 * model + k))
    return out


# ---- 6. rank deficiency ----------------------------------------------------------------------------------------------------------------
def _lines(board):
    ys = np.unique(board[:, 1])[::-1]
    xs = np.unique(board[:, 0])
    row = lambda k: np.nonzero(board[:, 1] == ys[k])[0]
    col = lambda k: np.nonzero(board[:, 0] == xs[k])[0]
    diag = np.nonzero(board[:, 0] == -board[:, 1])[0]
    assert len(ys) == 12 and len(xs) == 12 and len(diag) == 12 and len(row(3)) == 12 and len(col(7)) == 12
    return row, col, diag


@functools.lru_cache(maxsize=None)
def degenerate_frames():
    """(collinear, well-posed): five geometries whose corners do not span the board plane, each noise-free and at three seeds of
    0.1 px; and two nearly degenerate frames that do span it.  A row plus ONE corner of the next leaves a one-parameter family of
    homographies (those fixing the row's line pointwise are three, the extra corner takes two away): rank 7 of 8, as the yardstick
    confirms in tests/test_pose_init_cpu.py.  The smallest L that has a pose is a row plus TWO corners of the next."""
    board = board12()
    row, col, diag = _lines(board)
    R = tilted(600, 1)[0][0]
    t = look_at(R, board, DIST[EUCM], (0.03, -0.02))
    geo = [("row", row(9)), ("column", col(2)), ("diagonal", diag), ("one-corner", np.full(12, 77)),
           ("two-corners", np.array([5, 130] * 6))]
    bad = []
    for name, idx in geo:
        bad.append(frame(f"{name}-exact", EUCM, board, idx, R, t))
        for seed in (1, 2, 3):
            bad.append(frame(f"{name}-noise{seed}", EUCM, board, idx, R, t, noise_px=0.1, noise_seed=100 + seed))
    good = [frame("two-rows", EUCM, board, np.concatenate([row(3), row(4)]), R, t),
            frame("row-plus-two", EUCM, board, np.concatenate([row(3), row(4)[:2]]), R, t)]
    return bad, good


def row_plus_one():
    """The L of one row plus one corner of the next: rank-deficient (see degenerate_frames)."""
    board = board12()
    row, _, _ = _lines(board)
    R = tilted(600, 1)[0][0]
    return frame("row-plus-one", EUCM, board, np.concatenate([row(3), row(4)[:1]]), R, look_at(R, board, DIST[EUCM], (0.03, -0.02)))


def noisy_row_frame(pose6, seed=7):
    """One detected row of the default board seen from pose6 by the EUCM ground-truth camera, 0.1 px noise (the end-to-end case)."""
    board = board12()
    row, _, _ = _lines(board)
    return frame("row-e2e", EUCM, board, row(9), synth.rodrigues(np.asarray(pose6[:3])), np.asarray(pose6[3:], dtype=np.float64),
                 noise_px=0.1, noise_seed=200 + seed)


@functools.lru_cache(maxsize=None)
def e2e_session():
    """The 30-frame EUCM session of tests/test_gpu_init.py's test_calib_camera_without_initial_poses."""
    return synth.make_problem(30, "eucm")


def e2e_row_frame():
    """The frame the end-to-end case adds to that session: one noisy row seen from the session's first pose."""
    return noisy_row_frame(e2e_session().poses_gt[0])


# ---- 7. two cameras of different models ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def two_camera_frames():
    """4 slots x (KB4 camera 0, EUCM camera 1), the observations of a slot adjacent; each frame has a pose and a count of its own."""
    board = board12()
    out = []
    for cam, model in enumerate((KB4, EUCM)):
        Rs, offs = tilted(700 + cam, 4)
        for s, n in enumerate((144, 65, 30, 129)):
            f = frame(f"rig-cam{cam}-slot{s}", model, board, subset(board, n, 80 + 4 * cam + s), Rs[s], look_at(Rs[s], board, DIST[model], (offs[s], 0.0)))
            f["cam"], f["slot"] = cam, s
            out.append(f)
    return sorted(out, key=lambda f: (f["slot"], f["cam"]))


# ---- the lists, the yardstick on them, the measurement ---------------------------------------------------------------------------------
def well_posed_frames():
    """Every frame of the case list that is meant to have a pose at some min_points (the collinear ones are not among them)."""
    out = []
    for m in (UCM, EUCM, KB4, OPENCV5):
        out += lane_frames(m)
    out += rotation_frames() + count_frames(EUCM) + count_frames(DIVISION) + conditioning_frames() + noisy_frames()
    out += degenerate_frames()[1] + two_camera_frames()
    return out


def all_frames():
    return well_posed_frames() + degenerate_frames()[0]


_CACHE = {}


def reference(f, min_points=10):
    """The yardstick's answer for a frame: computed once, shared, never changed."""
    key = (f["name"], min_points)
    if key not in _CACHE:
        _CACHE[key] = ref.frame_pose(f["model"], f["params"], f["X"][:, 0], f["X"][:, 1], f["uv"], min_points)
    return _CACHE[key]


def emulation(f, min_points=10, tol=ref.PIVOT_TOL):
    return ref.emulate_f64(f["model"], f["params"], f["X"][:, 0], f["X"][:, 1], f["uv"], min_points, tol=tol)


def pose_errors(R, t, r):
    """(rotation, translation) error of a pose against the yardstick's dict r, each in units of kappa^2 u."""
    unit = r["kappa"] ** 2 * ref.U_F64
    return float(np.abs(R - r["R"]).max()) / unit, float(np.linalg.norm(t - r["t"]) / np.linalg.norm(r["t"])) / unit


def min_points_of(f):
    return 4 if f["name"].endswith("-four") else 10


def measure():
    """The figures behind F of tests/test_gpu_pose_init.py and PIVOT_TOL: printed and returned."""
    worst = (0.0, None)
    pivots = {}
    for f in well_posed_frames():
        r = reference(f, min_points_of(f))
        if r is None:
            continue                                             # 9 valid corners
        e = emulation(f, min_points_of(f))
        ratio = max(pose_errors(e["R"], e["t"], r))
        pivots[f["name"]] = r["min_rel_pivot"]
        if ratio > worst[0]:
            worst = (ratio, f["name"])
    low = min(pivots, key=pivots.get)
    print(f"emulate_f64 against solve over {len(pivots)} frames: worst err / (kappa^2 u) = {worst[0]:.3g} ({worst[1]})")
    print(f"smallest min_rel_pivot of a well-posed frame: {pivots[low]:.3g} ({low})")
    coll = {}
    for f in degenerate_frames()[0] + [row_plus_one()]:
        xn, yn, v = ref.unproject(f["model"], f["params"], f["uv"])
        s = ref.solve(f["X"][v, 0], f["X"][v, 1], xn[v], yn[v])
        coll[f["name"]] = (s["min_rel_pivot"], s["min_rel_pivot_mp"], emulation(f, tol=0.0))
    top = max(coll, key=lambda k: abs(coll[k][0]))
    print(f"largest |min_rel_pivot| of a frame that does not span the plane: long double {coll[top][0]:.3g} ({top})")
    slipped = [k for k, v in coll.items() if v[2]["used"] > 0]
    print(f"with the pivot test s > 0 the f64 emulation returns a pose for {len(slipped)} of {len(coll)}: {slipped}")
    for k in slipped:
        print(f"   {k}: emulated pivot {coll[k][2]['min_rel_pivot']:.3g}")
    return worst, pivots, coll


if __name__ == "__main__":
    measure()
