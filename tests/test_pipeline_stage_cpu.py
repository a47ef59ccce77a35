"""CPU: the caller thread's half of the streaming pipeline (csrc/pipeline_stage.h: feed checks, the fit test, the ring of launch
slots, the staging copies with the rollback of a refused feed, the answers' CSR, the result blocks' counts) as a stand-alone C++
program -- no device, no HIP.  tests/host/pipeline_stage_main.cpp drives the header in pipeline.hip's order against a model
(concatenate a launch's feeds, shift the rows), every staging buffer a heap block of exactly the pipeline's size.  Built twice:
plainly, and with -fsanitize=address,undefined (a host executable with its own main; nothing is preloaded)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]


def _cxx():
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx is not None, "no C++ compiler"
    return cxx


@pytest.mark.parametrize("flags", [[], SANITIZE], ids=["plain", "sanitized"])
def test_pipeline_stage_as_a_standalone_program(tmp_path, flags):
    cxx = _cxx()
    if flags:
        # can this compiler link and start the sanitizers' runtime at all?  (a one-line program tells)
        one = tmp_path / "one.cpp"
        one.write_text("int main() { return 0; }\n")
        probe = subprocess.run([cxx, *flags, str(one), "-o", str(tmp_path / "one")], capture_output=True, text=True)
        if probe.returncode != 0 or subprocess.run([str(tmp_path / "one")], capture_output=True).returncode != 0:
            pytest.skip("%s cannot link the sanitizer runtime: %s" % (cxx, probe.stderr.strip()[-200:]))
    exe = str(tmp_path / "pipeline_stage")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", *flags, "-I", os.path.join(ROOT, "spotify_recsys_challenge_2018_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "pipeline_stage_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout
