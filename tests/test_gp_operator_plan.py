"""The matrix-core gp_operator's kernel choice (csrc/kf_plan.h gp_operator_plan) and launch table, on the CPU."""
import pytest

import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.ops import kernels as K


def desc(op=K.OP_GP, d=4, frags=True):
    q = K.ext().BandDesc()
    q.op, q.d, q.map = op, d, list(range(d))
    q.gpm, q.gpm_nchunk = (4096, 2) if frags else (0, 0)
    return q


@pytest.mark.parametrize("n", (2, 3, 4, 7, 10))
@pytest.mark.parametrize("ds", ((2,), (3,), (4,), (7,), (10,), (4, 7), (2, 3, 4), (5,), (1,), (4, 6)))
@pytest.mark.parametrize("op,frags,device", ((K.OP_GP, True, True), (K.OP_GP, False, True), (K.OP_GP, True, False),
                                             (K.OP_LINEAR, True, True)))
def test_plan_is_matrix_core_exactly_under_the_rule(n, ds, op, frags, device):
    p = (ext := K.ext()).gp_operator_plan(n, [desc(d=ds[0])] + [desc(op, d, frags) for d in ds], device)
    want = device and frags and op == K.OP_GP and all(d in K.GP_OPERATOR_MFMA_D and d <= n for d in ds)
    assert p["family"] == (K.GP_OPERATOR_MFMA_KERNEL if want else "NONE")
    assert p["d"] == (sorted(ds) if want else []) and len(p["names"]) == len(p["d"])
    assert set(p["names"]) <= set(ext.gp_operator_table()) and not set(p["names"]) & set(ext.launch_table())
    assert p["resident"] == ([True] * (len(ds) + 1) if want else [])


def test_split_gp_is_validated():
    assert k.EngineConfig(split_gp="mfma").validate().split_gp == "mfma" and k.EngineConfig().split_gp == "valu"
    with pytest.raises(ValueError, match="split_gp"):
        k.EngineConfig(split_gp="x").validate()
