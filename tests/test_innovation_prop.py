"""The innovation check at the fused forecast off the device: ``ext.innovation_plan`` with ``prop``, the config
option, and the host runner's engine, where every date falls back to the materialised forecast."""
import json

import numpy as np
import pytest

import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.models.operators import _linear_device_spec
from kafka_inferenceengine_amd.ops import kernels as K

import kernel_cases as C
from test_innovation import engine_run, engine_setup, same_run
from test_innovation_mfma import GLOBAL, LDS, VALU, gp_table


@pytest.mark.parametrize("joint", [False, True])
@pytest.mark.parametrize("what,family,plain", [("tip", "innovation_prop_kernel", LDS), ("linear", "NONE", VALU),
                                               ("prosail5", "innovation_prop_g_kernel", GLOBAL)])
def test_plan_with_a_fused_forecast(what, family, plain, joint):
    if what == "prosail5":
        n, specs = 10, [k.gp_spec(em, range(10)) for em in k.make_prosail_emulators(n_bands=5, n_train=40, seed=0)]
    else:
        n, specs = 7, list(C.tip_problem(N=4, seed=8, n_train=60)["specs"])
        if what == "linear":
            specs.append(_linear_device_spec(7, k.LinearOperator(np.full(7, 0.1), 0.0), None, 0))
    tab = gp_table(specs, n, "cpu", np.full((len(specs), 4), 0.1), np.ones((len(specs), 4)))[0]
    p = K.innovation_plan(n, tab, joint, prop=True)
    assert (p["family"], p["joint"]) == (family, joint and family != "NONE"), p
    assert (p["name"] in K.ext().innovation_prop_table()) == (family != "NONE")
    assert p["name"] not in K.ext().innovation_table() and p["band_layout"] == (K.BAND_LAYOUT_SHARED_X if n == 10 else 0)
    assert K.innovation_plan(n, tab, joint)["family"] == plain      # without prop: the launches of before
    assert K.innovation_plan(n, tab, joint, prop=True, kind="covariance")["name"] == "NONE"
    assert "host twin" in K.innovation_prop_unsupported(n, tab, "cpu")


def test_config_option_and_host_engine_fallback(tmp_path):
    assert k.EngineConfig().innovation_forecast == "materialised"
    with pytest.raises(ValueError, match="innovation_forecast"):
        k.EngineConfig(innovation_forecast="lazy").validate()
    s = engine_setup(seed=4)
    path = tmp_path / "metrics.jsonl"
    a = engine_run(*s, analysis_form="information", innovation_gate=1.5, innovation_forecast="fused",
                   metrics_path=str(path))
    same_run(a, engine_run(*s, analysis_form="information", innovation_gate=1.5))
    per_date = [r["innovation"] for r in map(json.loads, open(path)) if r.get("event") == "date"]
    assert len(per_date) == 4 and all(m["forecast"] == "materialised" for m in per_date)
    assert int(a[0].gate_history.max()) >= 1
