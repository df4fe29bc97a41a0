"""CPU: the launch decisions of the Gram and eval launchers (csrc/ccal_gram_plan.hpp) through a plain C++ program
(tests/cpp/test_gram_plan.cpp) under the host's address and undefined-behaviour sanitizers.  The lane mapping and the fusion plan are
held, row by row, against tests/golden/gram_lane_plans.json: what the two cost models and the two copies of the fusion lines decided
before they became one (recorded from that commit's functions by a stand-alone program) - six kernel variants x 37 frame counts x 15
corner counts x 3 shares x 3 row caps = 29 970 rows, every lane mapping among the picks, plus forced mappings (each candidate, and 10,
which is ignored).  The dispatchers reach exactly the instantiation of their key and report a model or a mapping that is none."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
LANES = {"a": 6, "b": 8, "c": 12, "d": 16, "e": 32, "f": 64}


def _unrle(pairs):
    """run-length encoded list (a value, or [value, count] for a run) -> the values"""
    return [value for item in pairs for value, count in [item if isinstance(item, list) else (item, 1)] for _ in range(count)]


def _rows(table):
    grid = [(n, av, sh, mw) for n in table["n_obs"] for av in table["avg_corners"] for sh in table["share"] for mw in table["max_waves"]]
    for v in table["variants"]:
        key = (v["kernel"], v["two_per_simd"], v["general"])
        fuse, n_part = [_unrle(x) for x in v["fuse"]], [_unrle(x) for x in v["n_part"]]
        assert all(len(x) == len(grid) for x in [v["pick"]] + fuse + n_part)
        for i, point in enumerate(grid):
            yield key + point + (0, LANES[v["pick"][i]], fuse[0][i], n_part[0][i], fuse[1][i], n_part[1][i])
    for vi, n, av, sh, mw, forced, pick in table["forced"]:
        v = table["variants"][vi]
        yield (v["kernel"], v["two_per_simd"], v["general"], n, av, sh, mw, forced, pick, -1, 0, -1, 0)


def test_gram_plan_matches_recorded_decisions(tmp_path):
    with open(os.path.join(ROOT, "tests", "golden", "gram_lane_plans.json")) as f:
        table = json.load(f)
    rows = list(_rows(table))
    n_grid = 6 * 37 * 15 * 3 * 3
    assert n_grid == 29970 and len(rows) == n_grid + len(table["forced"]) and len(table["forced"]) >= 6 * 7
    assert {r[8] for r in rows[:n_grid]} == set(LANES.values())          # every mapping is chosen somewhere
    assert any(r[7] == 10 and r[8] != 10 for r in rows[n_grid:])
    path = tmp_path / "rows.txt"
    path.write_text("".join(" ".join(str(x) for x in r) + "\n" for r in rows))
    exe = str(tmp_path / "test_gram_plan")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Xarch_host", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "test_gram_plan.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe, str(path)], env=env, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and f"PLAN-OK {len(rows)} rows" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
