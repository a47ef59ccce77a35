"""CPU: the host-side validation of the titles a device-resident training set takes (csrc/train_feed_check.h
dae_train_titles_check, what dae_train_set_attach_titles refuses before any HIP call), as a stand-alone program."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_train_titles_validation_as_a_standalone_program(tmp_path):
    """tests/host/train_titles_check_main.cpp, compiled without the device: valid rows at L = 1, 25 and 64, a character id of
    n_char and of -2, L = 0 and L past the limit, rows for another number of playlists.  Exits 0 when all hold."""
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx is not None, "no C++ compiler"
    exe = str(tmp_path / "train_titles_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "spotify_recsys_challenge_2018_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "train_titles_check_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout
    for case in ("character id == n_char", "character id -2", "L = 0", "L = 65"):
        assert case in out.stdout
