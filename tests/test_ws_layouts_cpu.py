"""CPU: the layouts of the persistent blocks - a problem's inputs, the solver workspaces, the problem's scratch (csrc: ProblemLayout,
FusedLayout, GeneralLayout, NormalBaseLayout, PoseScratch, StatsScratch) - through a plain C++ program
(tests/cpp/test_ws_layouts.cpp) under the host's address and undefined-behaviour sanitizers.  The problem block and the fused
workspace's two blocks are held, offset by offset, against tests/golden/ws_layouts.json: what the size formulas and pointer walks of
ccal_problem_create and fused_ws_ensure gave before they became one declaration each (recorded once from verbatim copies of those
formulas by a stand-alone program), zero range, poison ranges and red_stride included.  The general workspace and the scratch layouts
are new: their properties are checked by the program itself."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ws_layouts") / "test_ws_layouts")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Xarch_host", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "test_ws_layouts.cpp"), "-o", out])
    return out


def test_problem_and_fused_layouts_match_recorded_offsets(exe):
    with open(os.path.join(ROOT, "tests", "golden", "ws_layouts.json")) as f:
        want = json.load(f)
    assert len(want) == 9 and sum("fused_dev" in c for c in want.values()) == 7
    out = subprocess.run([exe, "golden"], env=ENV, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    got = json.loads(out.stdout)
    assert list(got) == list(want)
    for name in want:
        assert got[name] == want[name], name
    # the cases reach what they are there for: a bin table, h_result absent above the spread limit and present at it
    assert want["ragged600_eucm"]["problem"]["bin_tab_bytes"] > 0 and want["empty"]["problem"]["bin_tab_bytes"] == 0
    assert want["poses_at_spread_limit"]["fused_host"]["h_result_bytes"] > 0 and want["poses_over_spread_limit"]["fused_host"]["h_result_bytes"] == 0


def test_general_and_scratch_layout_properties(exe):
    out = subprocess.run([exe, "check"], env=ENV, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "LAYOUT-OK" in out.stdout and "LAYOUT-FAIL" not in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
