"""``cli run --sensor s2 --in-decoder {host,device}``: on the CPU device the
"device" decoder is the host runner of the tile decoder (csrc/kf_inflate.h),
and the run equals the host reader's."""
import json
import os
import subprocess
import sys

import numpy as np

from kafka_inferenceengine_amd.input_output.synthetic import synthesize_s2_archive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="4")
    r = subprocess.run([sys.executable, "-m", "kafka_inferenceengine_amd", *args], capture_output=True, text=True,
                       timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_in_decoder_device_equals_host_on_cpu(tmp_path):
    data, emus, dates = synthesize_s2_archive(str(tmp_path / "arc"), np.ones((40, 300), bool), 2, 30, 0, "cpu", 0.1)
    recs = {}
    for mode in ("host", "device"):
        flag = ["--in-decoder", "device"] if mode == "device" else []      # the default is host
        recs[mode] = _run("run", "--sensor", "s2", "--s2-folder", data, "--emulator-folder", emus, "--device", "cpu",
                          *flag, "--out", str(tmp_path / mode), "--out-encoder", "host")
        assert recs[mode]["timesteps"] == 2 and recs[mode]["finite"]
    assert "ingest" not in recs["host"]
    ing = recs["device"]["ingest"]
    # 2 dates x 10 bands, each a 40 x 300 raster of 1 x 2 tiles: every file through the tile decoder
    assert ing["decoder"] == "device" and ing["files_host"] == 0 and ing["files_device"] == 20
    assert ing["tiles_device"] == 40 and 0 < ing["bytes_compressed_h2d"] < ing["bytes_h2d"]
    assert recs["host"]["gn_iterations"] == recs["device"]["gn_iterations"]
    names = sorted(os.listdir(tmp_path / "host"))
    assert names == sorted(os.listdir(tmp_path / "device")) and len(names) == 2 * 10 * 2
    for n in names:
        assert open(tmp_path / "host" / n, "rb").read() == open(tmp_path / "device" / n, "rb").read(), n


def test_in_decoder_defaults_to_host():
    """The readers default to the host decoder (the command line's default is
    pinned above: the run without the flag reports no device ingest)."""
    import inspect

    from kafka_inferenceengine_amd.input_output.sentinel import Sentinel2Observations
    from kafka_inferenceengine_amd.input_output.streaming import RasterIngest

    assert inspect.signature(Sentinel2Observations.__init__).parameters["decoder"].default == "host"
    assert inspect.signature(RasterIngest.__init__).parameters["decoder"].default == "host"
