"""``smooth_r1`` on the device: test_smoother_rank_one.py's checks at sizes around the wave and the workgroup,
with one workgroup walking the grid-stride loop, and the engine under ``smoother_form='rank_one'``."""
import pytest
import torch

from kafka_inferenceengine_amd.ops import kernels as K

from test_smoother_rank_one import SIZES, check_agreement, check_case, check_containment, check_engine, sweep

pytestmark = pytest.mark.gpu
cuda = torch.device("cuda")


@pytest.mark.parametrize("n", SIZES)
def test_smooth_r1_kernel_against_float64(n):
    sweep(check_case, n, (1, 63, 64, 65, 785), 2000 * n, cuda)
    sweep(check_agreement, n, (65,), 2000 * n, cuda)
    check_containment(n, 65, n, cuda)


@pytest.mark.parametrize("n", SIZES)
def test_smooth_r1_kernel_grid_stride_loop(n):
    """One workgroup for 785 pixels: every thread walks several pixels."""
    ext = K.ext()
    before = ext.get_max_blocks()
    ext.set_max_blocks(1)
    try:
        sweep(check_case, n, (785,), 3000 * n, cuda)
        check_containment(n, 785, n, cuda)
    finally:
        ext.set_max_blocks(before)


@pytest.mark.parametrize("form", ["information", "gain"])
def test_engine_rank_one_equals_dense_on_device(tmp_path, form):
    check_engine(tmp_path, form, device=cuda)
