"""The launch plan of the engine's forward (lightglue_amd/csrc/lg_forward_plan.h) is host arithmetic: tests/cpp/forward_plan_check.cpp walks the whole
decision table — layers x adaptive modes x keypoint counts around the pruning threshold x every fusion option x timing taps x debug stops — and asserts
the rules a forward has to keep (one producer per q/k/v, one final projection, no fusion across a row move, the debug step numbers).  No GPU."""
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_forward_plan_rules_hold_on_the_whole_grid(tmp_path):
    cxx = shutil.which("hipcc") or shutil.which("c++")
    assert cxx, "needs a C++17 host compiler (hipcc or c++)"
    exe = tmp_path / "forward_plan_check"
    src = ROOT / "tests" / "cpp" / "forward_plan_check.cpp"
    # -x c++: the header is host-only, so the program is built as plain C++ (no device pass)
    r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    assert int(r.stdout.split()[1]) > 100000, r.stdout   # the grid was walked
