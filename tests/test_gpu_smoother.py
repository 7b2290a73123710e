"""smooth_kernel on the device: the float64 truth and float32 yardstick of
test_smoother.py at sizes around the workgroup and with one workgroup walking
the grid-stride loop, the failure rule, and ``LinearKalman.smooth`` on the
device against the batch posterior, on the JRC-TIP headline configuration and
through the output classes."""
import numpy as np
import pytest
import torch

from kafka_inferenceengine_amd.ops import kernels as K

from test_smoother import (SIZES, check_engine_against_batch, check_engine_headline, check_failure_rule, check_kernel,
                           check_outputs)

pytestmark = pytest.mark.gpu
cuda = torch.device("cuda")


@pytest.mark.parametrize("n", SIZES)
def test_smooth_kernel_against_float64(n):
    for kappa in (10.0, 1e3):
        for N in (1, 63, 64, 65, 785):
            check_kernel(n, kappa, N, seed=10 * n + N + int(np.log10(kappa)), device=cuda)
    check_kernel(n, 1e3, 65, seed=3 * n, device=cuda, q_pix=True)
    check_failure_rule(n, 65, seed=n, device=cuda)


@pytest.mark.parametrize("n", SIZES)
def test_smooth_kernel_grid_stride_loop(n):
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


@pytest.mark.parametrize("form", ["information", "gain"])
def test_engine_smooth_equals_batch_posterior_on_device(tmp_path, form):
    check_engine_against_batch(tmp_path, form, device=cuda)


def test_engine_smooth_headline_configuration(tmp_path):
    """SyntheticBHRObservations on a 40 x 33 mask with holes, JRC-TIP, the LAI
    propagator with Q[6] = 0.04, 4 steps."""
    check_engine_headline(tmp_path, device=cuda, shape=(40, 33), steps=4)


def test_smoothed_output_files_equal_device_rasters_on_device(tmp_path):
    check_outputs(tmp_path, device=cuda, shape=(40, 33), steps=3)
