"""``gp_variance_kernel`` (csrc/kf_gp_variance.hip, ``K.gp_variance``) on the device against
the float64 ``variance`` within the allowance of gp_variance_cases.py, the containment of a
non-finite pixel, and the engine option ``emulator_uncertainty``.

N = 1: one lane; 65: one tile and a tail lane; 513: nine tiles on two workgroups
(grid-stride).  The leading dimension is N + 5 and the output's padding keeps a sentinel.

Measured on an MI355X, error over allowance: T = 500 JRC-TIP 0.56 / 0.43 / 0.24 and PROSAIL
0.06 / 0.48 / 0.37 for N = 1 / 65 / 513; the worst of the grid is JRC-TIP T = 31 N = 513,
0.998 (1.085e-6 s of 1.088e-6 s)."""
import numpy as np
import pytest
import torch

import gp_variance_cases as V
import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
PAD, SENTINEL = 5, -7.0


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


def _launch(c, dev, N, x=None):
    xd = torch.zeros((c["n"], N + PAD), device=dev)
    xd[:, :N] = torch.from_numpy(c["x"] if x is None else x).to(dev)
    out = torch.full((N + PAD,), SENTINEL, device=dev)
    K.gp_variance(c["n"], k.gp_spec(c["em"], c["smap"]), xd, out, N=N, grid=2 if N > 128 else None)
    out = out.cpu().numpy()
    assert (out[N:] == SENTINEL).all()
    return out[:N]


@pytest.mark.parametrize("N", (1, 65, 513))
@pytest.mark.parametrize("T", V.TS)
@pytest.mark.parametrize("layout", list(V.LAYOUTS))
def test_kernel_vs_float64(dev, layout, T, N):
    c = V.case(layout, T, N)
    V.check(f"kernel {layout} T={T} N={N}", c, _launch(c, dev, N))


@pytest.mark.parametrize("layout", list(V.LAYOUTS))
def test_non_finite_pixel_stays_contained(dev, layout):
    N, bad = 513, 100
    c = V.case(layout, 33, N)
    clean = _launch(c, dev, N)
    x = c["x"].copy()
    x[c["smap"][1], bad] = np.nan
    got = _launch(c, dev, N, x=x)
    others = np.arange(N) != bad
    assert np.isnan(got[bad]) and np.isfinite(clean).all()
    assert np.array_equal(got[others], clean[others])


def test_engine_option(dev):
    kf, st = V.engine_run(dev, emulator_uncertainty="report")
    std = kf.last_emulator_std
    assert std.shape == (2, st.N) and std.is_cuda and torch.equal(std, kf.emulator_variance())
    ref = np.sqrt(kf._last_date[1][0].emulator.variance(st.x[[0, 1, 6, 2], :st.N].T.double().cpu().numpy()))
    assert np.abs(std[0].cpu().numpy() - ref).max() < 1e-3 * ref.max()
    rec = [r for r in kf.metrics.records if r.get("event") == "date"][-1]["emulator"]
    assert len(rec) == 2 and all(r["max"] >= r["mean"] > 0 for r in rec)
    kf0, st0 = V.engine_run(dev)
    kf1, st1 = V.engine_run(dev, emulator_uncertainty="off")
    assert kf0.last_emulator_std is None and kf1.last_emulator_std is None
    for s in (st, st1):
        assert torch.equal(s.x, st0.x) and torch.equal(s.P, st0.P)
