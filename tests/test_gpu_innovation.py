"""innovation_kernel on the device: the float64 truth and bound of
test_innovation.py at sizes around the workgroup, the same checks again with
one workgroup for all pixels (the grid-stride loop), the device against the
host runner on every discrete output, and the engine's gate on the device."""
import numpy as np
import pytest
import torch

from kafka_inferenceengine_amd.ops import kernels as K

from test_innovation import (GROUPS5, NS, check_decisions, check_encodings, check_engine_gated_equals_edited,
                             check_engine_patch, check_failed_operator, check_failure_rule, check_gp, check_linear,
                             decisions_case, near_gate, rejected_of, run)
from test_marginal import SIZES

pytestmark = pytest.mark.gpu
cuda = "cuda"


@pytest.mark.parametrize("kind", K.MARGINAL_KINDS)
@pytest.mark.parametrize("nb", [1, 2, 10, 34])
@pytest.mark.parametrize("n", SIZES)
def test_linear_bands_against_float64(n, nb, kind):
    for i, N in enumerate(NS):
        check_linear(n, nb, N, kind, seed=100 * n + nb + i, device=cuda)


@pytest.mark.parametrize("scope", K.INNOVATION_SCOPES)
def test_screened_planes_and_decisions(scope):
    for N in NS:
        check_encodings(N, scope, device=cuda)
        for kind in K.MARGINAL_KINDS:
            check_decisions(N, kind, scope, seed=7, device=cuda)


@pytest.mark.parametrize("n", SIZES)
def test_failure_rule(n):
    for kind in K.MARGINAL_KINDS:
        check_failure_rule(n, 65, kind, device=cuda)
    if n == 2:
        for N in (1, 65, 785):
            check_failed_operator(N, device=cuda)


@pytest.mark.parametrize("kind", K.MARGINAL_KINDS)
def test_tip_gp_bands_against_float64_predict(kind):
    check_gp(kind, device=cuda)


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
                    check_linear(n, nb, N, kind, seed=100 * n + nb, device=cuda)
            check_failure_rule(n, 785, kind, device=cuda)
        if n == 4:
            for scope in K.INNOVATION_SCOPES:
                check_encodings(785, scope, device=cuda)
                check_decisions(785, "precision", scope, seed=7, device=cuda)
        if n == 7:
            check_gp("precision", device=cuda)
        if n == 2:
            check_failed_operator(785, device=cuda)
    finally:
        ext.set_max_blocks(before)
    assert ext.get_max_blocks() == before


@pytest.mark.parametrize("scope", K.INNOVATION_SCOPES)
@pytest.mark.parametrize("kind", K.MARGINAL_KINDS)
def test_device_equals_host_runner_on_discrete_outputs(kind, scope):
    """The same inputs through the kernel and the host runner: nobs, nrej, the
    screened planes and the NaN pattern agree wherever no |z| is within the z
    bound of the gate (there either rounding may decide)."""
    for N in NS:
        case, z64, bound = decisions_case(N, kind, seed=7)
        near = near_gate(case, z64, bound, 3.0, scope, GROUPS5)
        host = run(case, "cpu", gate=3.0, scope=scope, groups=GROUPS5, screened=True)
        dev = run(case, cuda, gate=3.0, scope=scope, groups=GROUPS5, screened=True)
        assert np.array_equal(np.isnan(host["z"]), np.isnan(dev["z"]))
        assert np.array_equal(host["nobs"], dev["nobs"]) and np.array_equal(host["status"], dev["status"])
        clear = ~near.any(axis=0)
        assert np.array_equal(host["nrej"][:N][clear], dev["nrej"][:N][clear])
        rh, rd = rejected_of(case, host), rejected_of(case, dev)
        assert np.array_equal(rh[~near], rd[~near])
        for b, (a, c) in enumerate(zip(host["screened"], dev["screened"])):
            keep = torch.from_numpy(~near[b])
            assert torch.equal(a[:N][keep], c[:N][keep]) and torch.equal(a[N:], c[N:])


@pytest.mark.parametrize("form,encoding,scope", [("information", "f32", "group"), ("gain", "dn16", "band")])
def test_engine_gated_run_equals_run_on_edited_source(form, encoding, scope):
    check_engine_gated_equals_edited(form, encoding, scope, device=cuda)


@pytest.mark.parametrize("form", ["information", "gain"])
def test_engine_gate_rejects_a_contaminated_patch(form):
    check_engine_patch(form, device=cuda)
