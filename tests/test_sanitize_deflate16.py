"""The 16-bit sample format of the tile encoder (csrc/kf_deflate.h: dfl_quantise,
DFL_FMT_U16) under AddressSanitizer + UBSan: a stand-alone program
(tests/native/sanitize_deflate16.cpp) runs the host runner in the fixed and the
dynamic-Huffman mode over a smooth, a constant, a noise, the adversarial and a
NaN tile and the padded shapes, with exactly-sized buffers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_deflate16_host_runner_under_asan_ubsan(tmp_path):
    exe = tmp_path / "sanitize_deflate16"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT}/csrc", "-fopenmp",
           f"{ROOT}/tests/native/sanitize_deflate16.cpp", f"{ROOT}/csrc/kf_host.cpp", "-lz", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, OMP_NUM_THREADS="2", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "sanitize_deflate16 ok" in r.stdout
