"""The float64 gp_operator's kernel choice (csrc/kf_plan.h gp_operator_f64_plan), launch table and config value, on
the CPU."""
import pytest

import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.ops import kernels as K


def desc(op=K.OP_GP, d=4):
    q = K.ext().BandDesc()
    q.op, q.d, q.map = op, d, list(range(d))
    return q


@pytest.mark.parametrize("n", (2, 4, 7, 10))
@pytest.mark.parametrize("ds", ((1,), (4,), (5,), (10,), (7, 4), (1, 5, 9), (11,), (0,)))
@pytest.mark.parametrize("op,groups,device", ((K.OP_GP, 2, True), (K.OP_GP, 0, True), (K.OP_GP, 2, False),
                                              (K.OP_LINEAR, 2, True)))
def test_plan_is_float64_exactly_under_the_rule(n, ds, op, groups, device):
    ext = K.ext()
    bands = [desc(d=ds[0])] + [desc(op, d) for d in ds]
    p = ext.gp_operator_f64_plan(n, bands, [2] + [groups] * len(ds), device)
    want = device and groups > 0 and op == K.OP_GP and all(1 <= d <= min(10, n) for d in ds)
    assert p["family"] == (K.GP_OPERATOR_F64_KERNEL if want else "NONE")
    assert p["nk"] == (sorted({(d + 3) // 4 for d in ds}) if want else []) and len(p["names"]) == len(p["nk"])
    others = set(ext.launch_table()) | set(ext.gp_operator_table())
    assert set(p["names"]) <= set(ext.gp_operator_f64_table()) and not set(ext.gp_operator_f64_table()) & others


def test_split_gp_f64_is_validated():
    assert k.EngineConfig(split_gp="f64").validate().split_gp == "f64"
    with pytest.raises(ValueError, match="split_gp"):
        k.EngineConfig(split_gp="x").validate()
