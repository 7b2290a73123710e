"""The joint instantiation of innovation_kernel on the device: the float64
truth and bound of test_evidence.py at sizes around the workgroup, the same
with one workgroup for all pixels (the grid-stride loop), JRC-TIP GP bands, the
device against the host runner, the other outputs' bits with and without the
joint outputs, and the engine's log evidence against the batch log density."""
import numpy as np
import pytest

from kafka_inferenceengine_amd.ops import kernels as K

from test_evidence import (NBS, check_engine_prediction_error_decomposition, check_high_snr, check_joint_failure_rule,
                           check_joint_gp, check_joint_linear, counted_of, e_joint, e_log, e_residual, joint_truth,
                           run_joint)
from test_innovation import NS, bits, linear_case
from test_marginal import SIZES

pytestmark = pytest.mark.gpu
cuda = "cuda"


@pytest.mark.parametrize("kind", K.MARGINAL_KINDS)
@pytest.mark.parametrize("nb", NBS)
@pytest.mark.parametrize("n", SIZES)
def test_joint_against_float64(n, nb, kind):
    for i, N in enumerate(NS):
        check_joint_linear(n, nb, N, kind, seed=100 * n + nb + i, device=cuda)


@pytest.mark.parametrize("kind", K.MARGINAL_KINDS)
@pytest.mark.parametrize("n,nb", [(1, 2), (3, 10), (7, 2), (10, 34)])
def test_joint_high_signal_to_noise(n, nb, kind):
    check_high_snr(n, nb, kind, device=cuda)


@pytest.mark.parametrize("kind", K.MARGINAL_KINDS)
def test_joint_tip_gp_bands_against_float64_predict(kind):
    check_joint_gp(kind, device=cuda)


@pytest.mark.parametrize("n", SIZES)
def test_joint_failure_rule(n):
    for kind in K.MARGINAL_KINDS:
        check_joint_failure_rule(n, 65, kind, device=cuda)


@pytest.mark.parametrize("n", SIZES)
def test_grid_stride_loop(n):
    """One workgroup for every launch: each thread walks several of the 785 pixels."""
    ext = K.ext()
    before = ext.get_max_blocks()
    ext.set_max_blocks(1)
    try:
        for kind in K.MARGINAL_KINDS:
            for nb in (2, 34):
                for N in (65, 785):
                    check_joint_linear(n, nb, N, kind, seed=100 * n + nb, device=cuda)
            check_joint_failure_rule(n, 785, kind, device=cuda)
        if n == 7:
            check_joint_gp("precision", device=cuda)
    finally:
        ext.set_max_blocks(before)
    assert ext.get_max_blocks() == before


@pytest.mark.parametrize("kind", K.MARGINAL_KINDS)
@pytest.mark.parametrize("n,nb", [(1, 1), (3, 5), (7, 2), (10, 34)])
def test_device_against_the_host_runner(n, nb, kind):
    """NaN pattern, nobs and status equal exactly; d2 / logdet within twice the
    bound (each side is within it of the float64 truth)."""
    for N in NS:
        case = linear_case(n, nb, N, kind, seed=13 + n)
        x, p = case["x"].clone(), case["p"].clone()
        if N > 2:      # an unscreenable pixel and a clean one next to it
            p[:, 1] = float("nan")
        host, dev = run_joint(case, "cpu", x=x, p=p), run_joint(case, cuda, x=x, p=p)
        for key in ("nobs", "status"):
            assert np.array_equal(host[key], dev[key]), key
        for key in ("d2", "logdet", "z"):
            assert np.array_equal(np.isnan(host[key]), np.isnan(dev[key])), key
        d64, _, _, _ = joint_truth(case)
        counted = counted_of(case)
        eJ, eres, elog = e_joint(case, counted), e_residual(case, counted), e_log(case, counted)
        ok = ~np.isnan(host["d2"][:N])
        assert ok.sum() >= N - 1
        assert np.all(np.abs(host["d2"][:N] - dev["d2"][:N])[ok] <= 2.0 * (eJ * d64 + eres)[ok])
        assert np.all(np.abs(host["logdet"][:N] - dev["logdet"][:N])[ok] <= 2.0 * (eJ + elog)[ok])


@pytest.mark.parametrize("kind", K.MARGINAL_KINDS)
def test_existing_outputs_unmoved(kind):
    """The joint instantiation writes the bits the plain one writes."""
    for n, nb, N in ((1, 1, 65), (3, 5, 785), (7, 2, 785), (10, 34, 257)):
        case = linear_case(n, nb, N, kind, seed=31 + n)
        groups = [b % 3 for b in range(nb)]
        a = run_joint(case, cuda, joint=True, gate=2.0, scope="group", groups=groups, screened=True)
        b = run_joint(case, cuda, joint=False, gate=2.0, scope="group", groups=groups, screened=True)
        for key in ("z", "chi2"):
            assert np.array_equal(a[key].view(np.int32), b[key].view(np.int32)), key
        for key in ("nobs", "nrej", "status"):
            assert np.array_equal(a[key], b[key]), key
        for s, t in zip(a["screened"], b["screened"]):
            assert bool((bits(s) == bits(t)).all())


@pytest.mark.parametrize("form", ["information", "gain"])
def test_engine_loglik_equals_batch_log_density(tmp_path, form):
    check_engine_prediction_error_decomposition(tmp_path, form, device=cuda, T=4)
