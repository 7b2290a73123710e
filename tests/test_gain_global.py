"""The gain form's global-table matrix-core kernel (kf_device.h
gain_mfma_g_kernel<10, 10, ...>: ten PROSAIL bands and the multi-sensor state,
whose tables exceed the LDS) in the built code objects: both observation
formats are there and each runs at >= 2 waves per SIMD, the budget of its
launch bound (VGPR + AGPR <= 256).  The scratch bytes per lane are printed,
not capped: the JRC-TIP gain kernel measured faster with a little scratch."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))

import isa_lint  # noqa: E402

# gain_mfma_g_kernel<NP = 10, D = 10, FOBS>(GainArgs): FOBS 1 = OBS_F32, 2 = OBS_DN16
KERNELS = {
    "f32": "_ZN2kf18gain_mfma_g_kernelILi10ELi10ELi1EEEvNS_8GainArgsE",
    "dn16": "_ZN2kf18gain_mfma_g_kernelILi10ELi10ELi2EEEvNS_8GainArgsE",
}


@pytest.fixture(scope="module")
def resources():
    sos = sorted((ROOT / "kafka_inferenceengine_amd").glob("_kafka_hip.*.so"))
    if not sos or not isa_lint.READELF.exists():
        pytest.skip("extension not built or llvm-readelf missing")
    return isa_lint.kernel_resources(sos[0])


@pytest.mark.parametrize("fobs", sorted(KERNELS))
def test_gain_global_kernel_is_built_at_two_waves(resources, fobs):
    name = KERNELS[fobs]
    assert name in resources, f"{name} not in the code objects"
    r = resources[name]
    vgpr, agpr = r["vgpr"], r.get("agpr", 0)
    print(f"gain_mfma_g_kernel<10,10,{fobs}>: {vgpr} VGPRs, {agpr} AGPRs, {r['scratch']} B scratch per lane, "
          f"{r.get('sgpr_spill', 0)} SGPR spills")
    assert vgpr + agpr <= 256, r
    assert isa_lint.waves_per_simd(vgpr, agpr) >= 2, r


def test_observation_format_codes_match_the_symbols():
    """The FOBS template arguments spelled in KERNELS are the wrapper's codes."""
    from kafka_inferenceengine_amd.ops import kernels as K

    assert (K.OBS_F32, K.OBS_DN16) == (1, 2)


def test_gain_prior_reset_stores_no_covariance_on_intermediate_dates(monkeypatch):
    """The S2 configuration on the host runner (SAIL prior reset, no
    propagator, gain form): the next forecast is PROP_PRIOR and reads nothing
    of the analysis, so under store_precision="auto" the intermediate dates
    launch with p_out = None (as the information form stores nothing) and the
    run equals store_precision="always"; the last date's covariance is full."""
    import datetime as dt

    import numpy as np
    import torch

    import kafka_inferenceengine_amd as k
    from kafka_inferenceengine_amd.ops import kernels as K

    mask = np.ones((20, 24), bool)
    mask[3:8, 2:11] = False
    dates = [dt.datetime(2017, 7, 3) + dt.timedelta(days=5 * i) for i in range(3)]
    grid = [dates[0] - dt.timedelta(days=1)] + [d + dt.timedelta(days=1) for d in dates]
    stores = []
    real_gain = K.gain

    def spy(n_params, bands, x_prev, x_f, p_f, x_out, p_out=None, *a, **kw):
        stores.append(p_out is not None)
        return real_gain(n_params, bands, x_prev, x_f, p_f, x_out, p_out, *a, **kw)

    monkeypatch.setattr(K, "gain", spy)

    def run(store):
        obs = k.SyntheticS2Observations(mask, dates=dates, n_bands=10, n_train=30, device="cpu", stream=False,
                                        n_pool=2, seed=5)
        prior = k.SAILPrior(k.SAIL_PARAMETERS, mask)
        out = k.DeviceOutput(k.SAIL_PARAMETERS)
        kf = k.LinearKalman(obs, out, mask, k.create_prosail_observation_operator, k.SAIL_PARAMETERS,
                            state_propagation=None, prior=prior, device="cpu",
                            config=k.EngineConfig(analysis_form="gain", store_precision=store))
        per_date = []
        real_do = kf.do_all_bands_state

        def do(*a, **kw):
            n0 = len(stores)
            res = real_do(*a, **kw)
            per_date.append((stores[n0:], res.state.p_valid))
            return res

        kf.do_all_bands_state = do
        st = kf.run(grid, kf.state_from_prior(prior), None, None)
        return st, out, per_date

    auto, oa, pa = run("auto")
    full, of, pf = run("always")
    assert len(pa) == len(pf) == len(dates)
    for launches, p_valid in pa[:-1]:
        assert launches and not any(launches) and p_valid == 0
    assert any(pa[-1][0]) and pa[-1][1] is None
    assert all(any(launches) and p_valid is None for launches, p_valid in pf)
    auto.require_full("the last date")
    assert torch.equal(auto.x, full.x) and torch.equal(auto.P, full.P)
    assert torch.equal(oa.mean, of.mean) and torch.equal(oa.unc, of.unc)
