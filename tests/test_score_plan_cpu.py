"""CPU: the plan of a ranking call (csrc/score_plan.h dae_plan_topk) as a stand-alone C++ program -- no device, no HIP.
tests/host/score_plan_main.cpp checks the function against the committed table of expected plans (tests/golden/
score_plans.txt: one case per branch, written by the planning arithmetic as it stood inline in the launch code) and, over a
grid of batch sizes, hidden sizes, image widths, k, dtypes, score mix and overlap hint, the conditions the launches rely on."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_score_plan_as_a_standalone_program(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx is not None, "no C++ compiler"
    exe = str(tmp_path / "score_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "spotify_recsys_challenge_2018_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "score_plan_main.cpp"), "-o", exe])
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "score_plans.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout
