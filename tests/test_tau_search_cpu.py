"""CPU: the threshold search of the fused scoring path (csrc/tau_search.h: dae_tau_search, dae_tau_key, dae_tau_value -- the
one copy both threshold kernels of csrc/tau_select.hip run) as a stand-alone C++ program -- no device, no HIP.
tests/host/tau_search_main.cpp feeds the search a brute-force counting functor over arrays of 0 .. 300 order-preserving keys
(random over several magnitudes, all equal, all -inf, a plateau that straddles the cut, keys that share their 16 leading bits;
need in {1, n - 1, n, n + 1, 1124}) and checks the prefix against an exhaustive scan, the "fewer than `need` keys" sentinel,
the 4-key slack rule and that the threshold never exceeds the element of rank `need`."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tau_search_as_a_standalone_program(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx is not None, "no C++ compiler"
    exe = str(tmp_path / "tau_search")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "spotify_recsys_challenge_2018_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "tau_search_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout
