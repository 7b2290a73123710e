"""pixel_product on the device: the float64 truth and bounds of test_product.py
at sizes around the workgroup, the grid-stride loop and the raster map, the
failure rule and the exact boundaries, host runner against device, the engine
with products and QA against the pass applied afterwards, and the files of the
device encoder."""
import datetime as dt

import numpy as np
import pytest
import torch

import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.ops import kernels as K

from test_marginal import SIZES
from test_product import (GT, Z95, assert_seen, check_boundaries, check_failure_rule, check_files, check_files_u16,
                          check_product, check_standard_planes_equal_unfused_run, engine_product_check, mixed_table,
                          new_seen, product_problem, run_product)

pytestmark = pytest.mark.gpu
cuda = torch.device("cuda")


@pytest.mark.parametrize("kind", ["precision", "covariance"])
@pytest.mark.parametrize("n", SIZES)
def test_product_kernel_against_float64(n, kind):
    seen = new_seen()
    for N in (1, 63, 64, 65, 785):
        check_product(n, N, seed=10 * n + N, kind=kind, device=cuda, seen=seen)
    assert_seen(seen)


@pytest.mark.parametrize("n", SIZES)
def test_product_kernel_failure_rule_and_boundaries(n):
    check_failure_rule(n, 65, seed=n, device=cuda)
    check_boundaries(device=cuda)


@pytest.mark.parametrize("n", SIZES)
def test_product_kernel_grid_stride_loop(n):
    """One workgroup for 785 pixels: every thread walks several pixels; the raster
    map goes into a plane of N + 5 cells whose other cells stay untouched
    (check_product: the float sentinel, 255 in QA)."""
    ext = K.ext()
    before = ext.get_max_blocks()
    ext.set_max_blocks(1)
    try:
        for kind in ("precision", "covariance"):
            check_product(n, 785, seed=7 * n, kind=kind, device=cuda)
        check_failure_rule(n, 785, seed=n, device=cuda)
    finally:
        ext.set_max_blocks(before)
    assert ext.get_max_blocks() == before


@pytest.mark.parametrize("kind", ["precision", "covariance"])
@pytest.mark.parametrize("n", SIZES)
def test_product_host_runner_and_device_agree(n, kind):
    """The same inputs on both runners: identical QA bytes and NaN pattern; the
    float planes are each within the bound of float64 (check_product on either),
    not bit-equal, because logf differs between the two."""
    N = 257
    table = mixed_table(n)
    x, p, idx, plane, _, _ = product_problem(n, N, 5 * n + 1, kind, table, Z95, bad=N // 2)
    rng = np.random.default_rng(n)
    status, nobs, nrej = (torch.from_numpy(rng.integers(0, 64, N).astype(np.uint8)),
                          torch.from_numpy(rng.integers(0, 3, N).astype(np.uint8)),
                          torch.from_numpy(rng.integers(0, 3, N).astype(np.uint8)))
    ph, qh = run_product(n, x, p, table, Z95, idx, plane, N, kind, status, nobs, nrej)
    pd, qd = run_product(n, x.to(cuda), p.to(cuda), table, Z95, idx.to(cuda), plane, N, kind, status.to(cuda),
                         nobs.to(cuda), nrej.to(cuda))
    assert np.array_equal(qh, qd)
    assert np.array_equal(np.isnan(ph), np.isnan(pd))
    check_product(n, N, 5 * n + 1, kind)
    check_product(n, N, 5 * n + 1, kind, device=cuda)


def _mask_with_holes(shape):
    mask = np.ones(shape, bool)
    mask[::7, 3::5] = False
    mask[:3, :4] = False
    return mask


def _tip_engine(mask, grid):
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
    return make


@pytest.mark.parametrize("form", ["information", "gain"])
def test_engine_product_output_on_device(form):
    mask = _mask_with_holes((40, 33))
    grid = [dt.datetime(2017, 1, 1) + dt.timedelta(days=16 * i) for i in range(4)]      # 3 dates
    out, _, _ = engine_product_check(form, _tip_engine(mask, grid))
    assert len(out.history) == 4            # the 3 dates and the timestep without one


def test_device_encoder_on_product_planes(tmp_path):
    mask = _mask_with_holes((300, 260))
    grid = [dt.datetime(2017, 1, 1) + dt.timedelta(days=16 * i) for i in range(2)]      # one date
    make = _tip_engine(mask, grid)
    check_files(tmp_path, make, "device", n_dates=1)
    check_files_u16(tmp_path, make, "device")


@pytest.mark.parametrize("form", ["information", "gain"])
def test_standard_planes_equal_unfused_run_on_device(form):
    mask = _mask_with_holes((40, 33))
    grid = [dt.datetime(2017, 1, 1) + dt.timedelta(days=16 * i) for i in range(4)]      # 3 dates
    check_standard_planes_equal_unfused_run(form, _tip_engine(mask, grid))


def test_qa_only_files_follow_their_timestep_with_the_device_encoder(tmp_path):
    """QA alone beside device-encoded standard rasters: the QA file of a timestep
    is written after that timestep's rasters and counted with them, so the
    rolling buffer (keep_timesteps) removes whole timesteps."""
    import os
    mask = _mask_with_holes((300, 260))
    grid = [dt.datetime(2017, 1, 1) + dt.timedelta(days=16 * i) for i in range(4)]      # 3 dates
    out = k.KafkaOutput(k.TIP_PARAMETERS, GT, "EPSG:32630", str(tmp_path), encoder="device", qa=True,
                        keep_timesteps=1)
    kf, run = _tip_engine(mask, grid)(out)
    run(kf)
    out.flush()
    ws = out.writer_stats()
    assert ws["deflate_backend"].startswith("device") and ws["timesteps_written"] == 3
    last = max(r["timestep"] for r in kf.history)
    day = dt.datetime.fromisoformat(last).strftime("A%Y%j")
    want = [f"{p}_{day}{s}.tif" for p in k.TIP_PARAMETERS for s in ("", "_unc")] + [f"QA_{day}.tif"]
    assert sorted(os.listdir(tmp_path)) == sorted(want)
    assert len(out.written) == 3 * 15
