"""marginal_kernel on the device: the float64 truth and bound of
test_marginal.py at sizes around the workgroup, the grid-stride loop, the
failure rule, the engine with marginal rasters against the non-fused
conditional run, and the device GeoTIFF encoder on marginal planes."""
import datetime as dt

import numpy as np
import pytest
import torch

import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.input_output.tiff import read_tiff
from kafka_inferenceengine_amd.ops import kernels as K

from test_marginal import SIZES, check_failure_rule, check_kernel, engine_pair

pytestmark = pytest.mark.gpu
cuda = torch.device("cuda")


@pytest.mark.parametrize("n", SIZES)
def test_marginal_kernel_against_float64(n):
    for N in (1, 63, 64, 65, 785):
        check_kernel(n, 1e3, N, seed=10 * n + N, device=cuda)
    check_failure_rule(n, 65, seed=n, device=cuda)


@pytest.mark.parametrize("n", SIZES)
def test_marginal_kernel_grid_stride_loop(n):
    """One workgroup for 785 pixels: every thread walks several pixels."""
    ext = K.ext()
    before = ext.get_max_blocks()
    ext.set_max_blocks(1)
    try:
        check_kernel(n, 1e3, 785, seed=7 * n, device=cuda)
        check_failure_rule(n, 785, seed=n, device=cuda)
    finally:
        ext.set_max_blocks(before)
    assert ext.get_max_blocks() == before


def _mask_with_holes(shape):
    mask = np.ones(shape, bool)
    mask[::7, 3::5] = False
    mask[:3, :4] = False
    return mask


@pytest.mark.parametrize("form", ["information", "gain"])
def test_engine_marginal_output_equals_non_fused_run_on_device(form):
    mask = _mask_with_holes((40, 33))
    grid = [dt.datetime(2017, 1, 1) + dt.timedelta(days=16 * i) for i in range(4)]      # 3 dates

    def make(out, **cfg):
        obs = k.SyntheticBHRObservations(mask, n_train=60, device=cuda, stream=False, n_pool=2, seed=1)
        kf = k.LinearKalman(obs, out, mask, k.create_nonlinear_observation_operator, k.TIP_PARAMETERS,
                            state_propagation=k.propagate_information_filter_LAI, device=cuda,
                            config=k.EngineConfig(**cfg))
        kf.set_trajectory_uncertainty(np.array([0, 0, 0, 0, 0, 0, 0.04]))

        def run(kf):
            st = kf.run(grid, kf.state_from_prior(k.JRCPrior(k.TIP_PARAMETERS, mask)), None, None)
            torch.cuda.synchronize()
            return st
        return kf, run

    om, _, _ = engine_pair(form, make, device=cuda)
    assert len(om.history) == 3


def test_device_encoder_on_marginal_planes(tmp_path):
    mask = _mask_with_holes((300, 260))
    grid = [dt.datetime(2017, 1, 1) + dt.timedelta(days=16 * i) for i in range(2)]      # one date

    def run(out):
        obs = k.SyntheticBHRObservations(mask, n_train=60, device=cuda, stream=False, n_pool=2, seed=1)
        kf = k.LinearKalman(obs, out, mask, k.create_nonlinear_observation_operator, k.TIP_PARAMETERS,
                            state_propagation=k.propagate_information_filter_LAI, device=cuda)
        kf.set_trajectory_uncertainty(np.array([0, 0, 0, 0, 0, 0, 0.04]))
        kf.run(grid, kf.state_from_prior(k.JRCPrior(k.TIP_PARAMETERS, mask)), None, None)
        torch.cuda.synchronize()

    ref = k.DeviceOutput(k.TIP_PARAMETERS, keep_history=True, uncertainty="marginal")
    run(ref)
    out = k.KafkaOutput(k.TIP_PARAMETERS, [0, 10, 0, 0, 0, -10], "EPSG:32630", str(tmp_path), encoder="device",
                        uncertainty="marginal")
    run(out)
    out.flush()
    ws = out.writer_stats()
    assert ws["deflate_backend"].startswith("device") and ws["uncertainty"] == "marginal"
    assert len(ref.history) == 1
    for ts, (m, u) in ref.history.items():
        assert torch.isfinite(u).all()
        for p, name in enumerate(k.TIP_PARAMETERS):
            core = f"{name}_{ts.strftime('A%Y%j')}"
            assert np.array_equal(read_tiff(tmp_path / f"{core}.tif")[0].reshape(-1), m[p].cpu().numpy())
            arr, info = read_tiff(tmp_path / f"{core}_unc.tif")
            assert np.array_equal(arr.reshape(-1), u[p].cpu().numpy()) and info["uncertainty"] == "marginal"
