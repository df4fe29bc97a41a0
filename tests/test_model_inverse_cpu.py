"""CPU: what tests/model_inverse_cases.py claims, on the mpmath reference of tests/model_inverse_ref.py alone - the conditions the
INPUTS of tests/test_gpu_model_inverse.py have to meet, whatever the kernels do - and the proof that the GPU test had something to
find: the two published KB4 loops, replayed in plain f64 WITHOUT an acceptance check, return rays on these cases that do not
re-project onto their pixel."""
import collections

import mpmath as mp
import numpy as np
import pytest

import model_inverse_cases as cases
import model_inverse_ref as ref

UCM, EUCM, KB4, OPENCV5 = ref.UCM, ref.EUCM, ref.KB4, ref.OPENCV5


def _classes(model_list, normalized):
    cnt = collections.Counter()
    for c in cases.CASES:
        if c.model in model_list:
            cnt.update(r.cls for r in c.reference(normalized))
    return cnt


def test_launch_sizes_and_sets():
    sizes = collections.Counter(c.size for c in cases.CASES)
    assert set(sizes) == {1, 63, 64, 65, 257, 1000} and sizes[1000] == 1, sizes
    for c in cases.CASES:
        assert len(c.unique) % 2 == 1 and c.inputs().shape == (c.size, 2)
    alphas = {float(c.params[4]) for c in cases.of_model(EUCM)}
    assert {1e-6, 0.3, 0.5, 0.5 + 2.0 ** -30, 0.9, 1.0} <= alphas and len(cases.of_model(EUCM)) >= 28
    assert any(c.params[0] != c.params[1] and abs(c.params[0] - c.params[1]) > 1.0 for c in cases.of_model(UCM))
    assert sum(c.name.startswith("kb4_draw_") for c in cases.CASES) == 32
    assert sum(c.folding for c in cases.CASES) >= 10


@pytest.mark.parametrize("normalized", [False, True])
def test_kb4_class_shares(normalized):
    cnt = _classes((KB4,), normalized)
    n = sum(cnt.values())
    print(f"KB4 normalized={normalized}: {dict(cnt)} of {n} unique rows")
    assert cnt["A"] >= 0.40 * n and cnt["B"] >= 0.15 * n and cnt["C"] <= 0.25 * n, cnt


@pytest.mark.parametrize("normalized", [False, True])
def test_near_rows_are_rare_and_the_edge_row_is_one(normalized):
    cnt = _classes((UCM, EUCM), normalized)
    n = sum(cnt.values())
    print(f"UCM / EUCM normalized={normalized}: {dict(cnt)} of {n} unique rows")
    assert cnt["near"] <= 0.001 * n, cnt
    assert cnt["C"] == 0
    for name in ("ucm_edge", "eucm_edge"):
        c = cases.by_name(name)
        assert tuple(c.unique[c.edge]) == cases.EDGE_ROW and c.reference(normalized)[c.edge].cls == "near"
        mx = c.unique[c.edge][0] / c.params[0]
        assert mx * mx == 1.0                                                   # r^2 == the limit, no rounding


@pytest.mark.parametrize("normalized", [False, True])
def test_every_set_has_an_A_row_and_every_folding_set_a_B_row(normalized):
    for c in cases.CASES:
        cls = [r.cls for r in c.reference(normalized)]
        assert "A" in cls, c.name
        if c.folding:
            assert "B" in cls, c.name
        if c.model == OPENCV5:
            assert "B" not in cls
    zeros = [r.cls for r in cases.by_name("kb4_zeros").reference(normalized)]
    assert "B" in zeros                                                         # r > pi: the `t >= pi` branch
    # the limit rows: (1 - 1e-3) and (1 - 1e-9) inside, (1 + 1e-3) and (1 + 1e-9) outside
    for c in cases.CASES:
        if c.model in (UCM, EUCM) and c.params[4] > 0.5 and not c.name.endswith(("_edge", "_one_row")):
            assert [r.cls for r in c.reference(False)[3:7]] == ["A", "B", "A", "B"], c.name
    # the folding rows: r_c (1 - 1e-3) and r_c (1 - 1e-6) have a root, r_c (1 + 1e-3) and r_c (1 + 1e-6) have none before the fold
    for c in cases.CASES:
        if c.folding and c.name != "kb4_zeros":
            ks = ref.kb4_set(c.params)
            with mp.workdps(ref.DPS):
                for j, below in zip(range(3, 7), (True, False, True, False)):
                    m = (mp.mpf(c.unique[j][0]) - mp.mpf(c.params[2])) / mp.mpf(c.params[0]), (mp.mpf(c.unique[j][1]) - mp.mpf(c.params[3])) / mp.mpf(c.params[1])
                    r = mp.sqrt(m[0] ** 2 + m[1] ** 2)
                    first = [t for t in ks.roots(r) if t <= ks.fold[0]]
                    assert bool(first) == below, (c.name, j)


def test_round_trip_of_the_reference():
    """project_mp(the reference's ray) == the pixel to 1e-40 on every A row: the two halves of the yardstick agree"""
    worst = 0.0
    for c in cases.CASES:
        rows = c.reference(False)
        idx = [i for i, r in enumerate(rows) if r.cls == "A"]
        with mp.workdps(ref.DPS):
            for i in idx:
                uv, valid, _ = _project_exact(c.model, c.params, rows[i].ray)
                assert valid, (c.name, i)
                err = max(abs(uv[0] - mp.mpf(c.unique[i][0])), abs(uv[1] - mp.mpf(c.unique[i][1])))
                worst = max(worst, float(err))
                assert err < mp.mpf(10) ** -40, (c.name, i, float(err))
    print(f"round trip of the reference: worst {worst:.3e} px")


def _project_exact(model, p, ray):
    """project_mp on an mpf ray (project_mp takes doubles): the same definitions, through its own helpers"""
    q = ref._params(p)
    x, y, z = ray
    r2 = x * x + y * y
    if model in (UCM, EUCM):
        alpha, beta = q[4], (q[5] if model == EUCM else mp.mpf(1))
        d = mp.sqrt(beta * r2 + z * z)
        w = alpha / (1 - alpha) if alpha <= mp.mpf(0.5) else (1 - alpha) / alpha
        nrm = alpha * d + (1 - alpha) * z
        return (q[0] * (x / nrm) + q[2], q[1] * (y / nrm) + q[3]), z + w * d >= -mp.mpf(10) ** -45, False
    if model == KB4:
        r = mp.sqrt(r2)
        if r > ref.SMALL_RADIUS:
            td = ref._kb4_g(q[4:8], mp.atan2(r, z))
            return (q[0] * (td * x / r) + q[2], q[1] * (td * y / r) + q[3]), True, False
        return (q[0] * (x / z) + q[2], q[1] * (y / z) + q[3]), True, False
    mx, my = ref._ocv5_forward(q[4:9], x / z, y / z)
    return (q[0] * mx + q[2], q[1] * my + q[3]), z > mp.mpf(1e-9), False


def test_project_mp_agrees_with_its_exact_form_on_doubles():
    """project_mp (doubles in) against _project_exact above on the same points, and its validity against undistort_ref's f64 rule"""
    import undistort_ref
    for c, rays in cases.project_cases()[:6]:
        uv, valid, near = cases.project_reference(c, rays)
        v64, _ = undistort_ref.project_valid(c.model, c.params, rays)
        assert np.array_equal(valid[~near], v64[~near])
        with mp.workdps(ref.DPS):
            for i in np.nonzero(valid)[0][:20]:
                e, _, _ = _project_exact(c.model, c.params, tuple(mp.mpf(float(v)) for v in rays[i]))
                assert abs(e[0] - uv[i][0]) + abs(e[1] - uv[i][1]) < mp.mpf(10) ** -40


def test_project_inputs():
    """the project cases: the rays within BOUNDARY_REL of a validity boundary stay under the cap over all cases together (and are
    the back axis at alpha = 1/2, which lies on the boundary exactly), both answers occur, alpha <= 1/2 included"""
    small_alpha, n_near, n = 0, 0, 0
    for c, rays in cases.project_cases():
        uv, valid, near = cases.project_reference(c, rays)
        n_near += int(near.sum()); n += len(rays)
        assert near.sum() == (1 if c.params[4] == 0.5 and c.model in (UCM, EUCM) else 0), c.name
        assert valid.any(), c.name
        if c.model != KB4:
            assert (~valid).any(), c.name
        small_alpha += c.model in (UCM, EUCM) and c.params[4] <= 0.5
    print(f"project: {n_near} near rows of {n}")
    assert n_near <= 0.001 * n and small_alpha >= 15


# ---- the published KB4 loops in plain f64, without an acceptance check ----------------------------------------------------------------
def _replay_kb4(p, uv, steps, stop, t_max):
    """(t, r, valid) of the loop as it was published: `steps` Newton steps from t = r, valid iff 0 < t < t_max"""
    mx, my = (uv[:, 0] - p[2]) / p[0], (uv[:, 1] - p[3]) / p[1]
    r = np.sqrt(mx * mx + my * my)
    t = r.copy()
    done = np.zeros(len(r), dtype=bool)
    with np.errstate(all="ignore"):
        for _ in range(steps):
            t2 = t * t
            f = t * (1.0 + t2 * (p[4] + t2 * (p[5] + t2 * (p[6] + t2 * p[7])))) - r
            fp = 1.0 + t2 * (3.0 * p[4] + t2 * (5.0 * p[5] + t2 * (7.0 * p[6] + t2 * 9.0 * p[7])))
            dt = f / fp
            t = np.where(done, t, t - dt)
            if stop:
                done |= np.abs(dt) < 1e-14
        t2 = t * t
        res = np.abs(t * (1.0 + t2 * (p[4] + t2 * (p[5] + t2 * (p[6] + t2 * p[7])))) - r)
        valid = (t > 0.0) & (t < t_max) & (r >= ref.SMALL_RADIUS)
    return res, valid


@pytest.mark.parametrize("which, steps, stop, t_max", [("unproject_ray", 20, True, np.pi), ("unproject_normalized", 10, False, 1.5)])
def test_the_unchecked_kb4_loop_is_unsound_on_these_cases(which, steps, stop, t_max):
    unsound, b_valid, a_lost, n = 0, 0, 0, 0
    for c in cases.of_model(KB4):
        res, valid = _replay_kb4(c.params, c.unique, steps, stop, t_max)
        cls = np.array([r.cls for r in c.reference(which == "unproject_normalized")])
        small = np.array([r.small for r in c.reference(which == "unproject_normalized")])
        unsound += int((valid & ~(res <= 1e-9)).sum())
        b_valid += int((valid & (cls == "B")).sum())
        a_lost += int(((cls == "A") & ~small & ~(valid & (res < 1e-9))).sum())
        n += len(res)
    print(f"{which} replayed without the acceptance check: {unsound} unsound rows of {n}, {b_valid} of them on B rows; "
          f"A rows the checked loop would lose: {a_lost}")
    assert unsound > 0 and b_valid > 0
    assert a_lost == 0                      # with the check, the f64 loop still returns every A row: the classes leave it room
