"""The matrix-core innovation check off the device: ``ext.innovation_plan``, the refusals, the engine's fallback."""
import numpy as np
import pytest
import torch

import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.engine.bands import DeviceBand, RecordCache, build_table
from kafka_inferenceengine_amd.models.operators import _sar_device_spec
from kafka_inferenceengine_amd.ops import kernels as K

import kernel_cases as C
from test_innovation import engine_run, engine_setup, same_run

LDS, GLOBAL, VALU = "innovation_mfma_kernel", "innovation_mfma_g_kernel", "pixel_kernel"


def gp_table(specs, n, device, y, w):
    obs = [DeviceBand(K.OBS_F32, y=torch.tensor(a, dtype=torch.float32, device=device),
                      w=torch.tensor(b, dtype=torch.float32, device=device)) for a, b in zip(y, w)]
    return build_table(specs, obs, n, RecordCache(), device), obs


@pytest.mark.parametrize("what,n,gp,family,layout", [
    ("tip", 7, "mfma", LDS, 0), ("prosail3", 10, "mfma", GLOBAL, K.BAND_LAYOUT_SHARED_X),
    ("prosail5", 10, "mfma", GLOBAL, K.BAND_LAYOUT_SHARED_X), ("sar", 7, "mfma", VALU, 0), ("tip", 4, "mfma", VALU, 0),
    ("tip", 7, "valu", VALU, 0), ("no_fragments", 7, "mfma", VALU, 0)])
@pytest.mark.parametrize("joint", [False, True])
def test_plan_rules(what, n, gp, family, layout, joint):
    if what.startswith("prosail"):
        specs = [k.gp_spec(em, range(10)) for em in k.make_prosail_emulators(n_bands=int(what[-1]), n_train=40, seed=0)]
    else:
        specs = list(C.tip_problem(N=4, seed=8, n_train=60)["specs"])
        if what == "sar":
            specs.append(_sar_device_spec(7, None, None, 0, band_mapper=[[6, 0]]))
    tab = gp_table(specs, max(n, 7), "cpu", np.full((len(specs), 4), 0.1), np.ones((len(specs), 4)))[0]
    for d in tab.descs if what == "no_fragments" else ():
        d.gpm_nchunk = 0
    p = K.innovation_plan(n, tab, joint, gp)
    assert (p["family"], p["band_layout"], p["joint"], p["np"]) == (family, layout, joint, n), p
    assert (p["name"] in K.ext().innovation_table()) == (family != VALU)
    assert K.innovation_mfma_supported(n, tab, "cpu") is False


def test_refusals():
    tab = gp_table(C.tip_problem(N=4, seed=8, n_train=60)["specs"], 7, "cpu", np.zeros((2, 4)), np.ones((2, 4)))[0]
    x, p, st = torch.zeros(7, 4), torch.zeros(28, 4), torch.zeros(4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="host twin"):
        K.innovation(7, tab, x, p, kind="precision", status=st, gp="mfma")
    with pytest.raises(ValueError, match="gp must be"):
        K.innovation(7, tab, x, p, kind="precision", status=st, gp="x")
    with pytest.raises(ValueError, match="innovation_gp"):
        k.EngineConfig(innovation_gp="x").validate()


def test_cpu_engine_falls_back_to_the_valu_kernel_bit_for_bit():
    s = engine_setup(seed=4)
    a = engine_run(*s, analysis_form="information", innovation_gate=1.5, innovation_gp="mfma")
    same_run(a, engine_run(*s, analysis_form="information", innovation_gate=1.5))
    assert int(a[0].gate_history.max()) >= 1
