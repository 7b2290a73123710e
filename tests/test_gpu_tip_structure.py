"""The JRC-TIP kernels with the structure-aware solve (SPEC_*_TIP, kf_core.h
StructTip) and the unobserved-wave shortcut (kf_gp_mfma.h) against the dense
kernels: the forced-dense variant (everything else equal, line tables on) and
the generic launch (variant 18, line tables off).  Every skipped operation has
an exact zero factor and an unobserved wave's analysis is its forecast, so the
results are equal bit for bit."""
from __future__ import annotations

import datetime as dt
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.ops import kernels as K

ROOT = Path(__file__).resolve().parents[1]

N_DATES = 4
N_POOL = 3


def _mask():
    mask = np.ones((23, 17), bool)
    mask[4:7, 5:9] = False     # 391 - 12 = 379 pixels: five whole waves and one of 59
    return mask


def _run(cuda, n_train, variant, line, spatial=False):
    mask = _mask()
    # the first time of the grid starts the run: N_DATES analysis dates follow it
    grid = [dt.datetime(2017, 1, 1) + dt.timedelta(days=16 * i) for i in range(N_DATES + 1)]
    old, old_line = K.DEFAULT_VARIANT, K.LINE_TABLES
    K.DEFAULT_VARIANT, K.LINE_TABLES = variant, line
    K.STRUCT_LAUNCHES.update(tip=0, dense=0)
    try:
        out = k.DeviceOutput(k.TIP_PARAMETERS, keep_history=True)
        # cloud cells of 4 pixels over 45 % of the pixels: 230 to 242 of the 379 pixels observed per date,
        # so the fourth wave is mixed and the last two hold unobserved pixels only (asserted by the test)
        obs = k.SyntheticBHRObservations(mask, n_train=n_train, device=cuda, stream=False, n_pool=N_POOL,
                                         field_cell=8, cloud_fraction=0.45)
        cfg = dict(spatial_gamma=5.0, spatial_params=[6]) if spatial else dict(convergence_chunk=[8, 8])
        kf = k.LinearKalman(obs, out, mask, k.create_nonlinear_observation_operator, k.TIP_PARAMETERS, device=cuda,
                            state_propagation=k.propagate_information_filter_LAI, config=k.EngineConfig(**cfg))
        kf.set_trajectory_uncertainty(np.array([0, 0, 0, 0, 0, 0, 0.04]))
        st = kf.run(grid, kf.state_from_prior(k.JRCPrior(k.TIP_PARAMETERS, mask)), None, None)
        torch.cuda.synchronize()
        n_obs = [int((obs._pool[p] != 0).any(0).sum()) for p in range(N_POOL)]
        return dict(x=st.x.cpu(), P=st.P.cpu(), status=kf.last_status.cpu(), N=int(st.N), n_obs=n_obs,
                    norms=[h.get("norms") for h in kf.history], iters=[h.get("gn_iterations") for h in kf.history],
                    chunk_iters=[h.get("chunk_iters") for h in kf.history],
                    rasters={t: (m.cpu(), u.cpu()) for t, (m, u) in out.history.items()},
                    launches=dict(K.STRUCT_LAUNCHES))
    finally:
        K.DEFAULT_VARIANT, K.LINE_TABLES = old, old_line


def _same(a, b):
    assert a["iters"] == b["iters"] and a["chunk_iters"] == b["chunk_iters"] and a["norms"] == b["norms"]
    assert torch.equal(a["x"], b["x"]) and torch.equal(a["P"], b["P"]) and torch.equal(a["status"], b["status"])
    assert a["rasters"].keys() == b["rasters"].keys() and len(a["rasters"]) == N_DATES
    for t in a["rasters"]:
        assert torch.equal(a["rasters"][t][0], b["rasters"][t][0]), t
        assert torch.equal(a["rasters"][t][1], b["rasters"][t][1]), t


# T = 33: the peeled chunk and one pass of the chunk loop; T = 32: one chunk
# (both the small-emulator kernel, SPEC_PROP_PF_TIP); T = 160: more than four
# chunks per band, the headline kernel (SPEC_PROP_TIP)
@pytest.mark.gpu
@pytest.mark.parametrize("n_train", [33, 32, 160])
def test_structure_aware_kernels_equal_dense(cuda, n_train):
    got = _run(cuda, n_train, K.Variant.DEFAULT, True)
    # dates 2..4 take the fused forecast (the first has none): the structure-aware kernels ran
    assert got["launches"]["tip"] >= N_DATES - 1 and got["launches"]["dense"] == 0, got["launches"]
    # the observed-first order puts n_obs observed pixels ahead of the others: on
    # every date some wave holds unobserved pixels only (the shortcut) and one
    # holds both kinds (the full path next to it)
    N = got["N"]
    assert N == 379 and N % 64 != 0
    for n_obs in got["n_obs"]:
        first_clear = -(-n_obs // 64) * 64      # first slot of the first wave past the observed pixels
        assert first_clear < N, (n_obs, N)                 # a wave without any observation
        assert n_obs % 64 != 0 and 0 < n_obs < N, n_obs    # a mixed wave
    assert (got["status"][:N] & K.ST_NO_OBS).any() and not (got["status"][:N] & K.ST_FALLBACK).any()
    dense = _run(cuda, n_train, K.Variant.DENSE_SOLVE, True)
    assert dense["launches"]["tip"] == 0, dense["launches"]
    _same(got, dense)
    got_nl = _run(cuda, n_train, K.Variant.DEFAULT, False)
    generic = _run(cuda, n_train, K.Variant.GENERIC_SPEC, False)
    assert got_nl["launches"]["tip"] >= N_DATES - 1 and generic["launches"]["tip"] == 0
    _same(got_nl, generic)


@pytest.mark.gpu
def test_structure_aware_spatial_kernel_equals_dense(cuda):
    """The regulariser-prepare twin (SPEC_PROP_REG_TIP): the structure-aware
    factorisation also serves the V = A_reg^-1 E_R solves."""
    got = _run(cuda, 160, K.Variant.DEFAULT, True, spatial=True)
    assert got["launches"]["tip"] >= N_DATES - 1, got["launches"]
    dense = _run(cuda, 160, K.Variant.DENSE_SOLVE, True, spatial=True)
    assert dense["launches"]["tip"] == 0, dense["launches"]
    _same(got, dense)


def test_structure_aware_kernels_keep_the_headline_budget():
    """The new instantiations run at the parent headline kernel's budget: at
    least 3 waves per SIMD and no scratch."""
    sys.path.insert(0, str(ROOT / "tools"))
    import isa_lint

    so = ROOT / "kafka_inferenceengine_amd" / "_kafka_hip.cpython-310-x86_64-linux-gnu.so"
    if not so.exists() or not isa_lint.READELF.exists():
        pytest.skip("extension not built or llvm-readelf missing")
    res = isa_lint.kernel_resources(so)
    for spec in (4, 5, 6):     # SPEC_PROP_TIP, SPEC_PROP_REG_TIP, SPEC_PROP_PF_TIP
        name = f"_ZN2kf20analysis_mfma_kernelILi7ELi4ELi2ELi256ELi3ELi1ELb1ELi{spec}EEEvNS_12AnalysisArgsE"
        assert name in res, f"{name} not in the code objects"
        r = res[name]
        assert isa_lint.waves_per_simd(r["vgpr"], r.get("agpr", 0)) >= 3, (name, r)
        assert r["scratch"] == 0, (name, r)
