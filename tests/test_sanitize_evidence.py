"""The joint innovation statistic's per-pixel code (csrc/kf_core.h
``pixel_innovation<NP, true>``) under AddressSanitizer + UBSan: a stand-alone
program (tests/native/sanitize_evidence.cpp) runs the host runner at every
compiled state size, both kinds, 1 to 64 bands, with exactly-sized buffers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_joint_innovation_host_runner_under_asan_ubsan(tmp_path):
    exe = tmp_path / "sanitize_evidence"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT}/csrc", "-fopenmp",
           f"{ROOT}/tests/native/sanitize_evidence.cpp", f"{ROOT}/csrc/kf_host.cpp", "-lz", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, OMP_NUM_THREADS="2", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "sanitize_evidence ok" in r.stdout
