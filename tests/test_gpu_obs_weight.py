"""``gp_obs_weight_kernel`` (csrc/kf_gp_variance.hip, ``K.gp_variance(obs=...)``) on the device against
float64 (reference and bound: test_obs_weight.py), the skipped tile and the batched launch, the
containment of a non-finite pixel, and ``emulator_uncertainty='inflate'``.

N = 1: one lane; 65: one tile and a tail tile of one unobserved pixel; 513: nine tiles on two workgroups
per band (grid-stride), the tile 64..127 without an observation.

Measured on an MI355X, worst error over bound: 0.83 (JRC-TIP, F32 + mask, N = 65); T = 500: 0.43; the
PROSAIL cases stay below 0.22.  w'/w is 0.003 .. 0.41 in the mean, so w' = w would miss every case."""
import numpy as np
import pytest
import torch

import gp_variance_cases as V
import kafka_inferenceengine_amd as k
import test_obs_weight as W
from kafka_inferenceengine_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [(lay, enc, 33, N) for lay in V.LAYOUTS for enc in W.ENCODINGS for N in (1, 65, 513)] + \
    [("tip", "dn16", 500, 65)]


def _grid(N):
    return dict(grid=2) if N > 128 else {}


def _tiles_seen(db, N):
    """Pixels of the 64-pixel tiles that hold an observation: where the kernel evaluates the variance."""
    seen = np.zeros(-(-N // 64) * 64, bool)
    seen[:N] = db.decode()[1][:N].cpu().numpy() > 0
    return np.repeat(seen.reshape(-1, 64).any(1), 64)[:N]


@pytest.mark.parametrize("layout,encoding,T,N", CASES)
def test_kernel_vs_float64(layout, encoding, T, N):
    c, db = V.case(layout, T, N), W.band(encoding, N, DEV)
    out = W.launch(c, db, N, DEV, **_grid(N))
    at = _tiles_seen(db, N)
    W.check(f"kernel {layout} {encoding} T={T} N={N}", c, db, out, at)
    assert not out[1:, ~at].any()


def test_unobserved_tile_and_batched_bands():
    N = 513
    ems = k.make_tip_emulators(n_train=33)
    specs = [k.gp_spec(ems[0], [0, 1, 6, 2]), k.gp_spec(ems[1], [3, 4, 6, 5])]
    dbs = [W.band("dn16", N, DEV), W.band("f32mask", N, DEV)]
    x = torch.zeros((7, N + W.PAD), device=DEV)
    x[:, :N] = torch.from_numpy(V.case("tip", 33, N)["x"]).to(DEV)
    both, one = torch.zeros((2, 3, N), device=DEV), torch.zeros((2, 3, N), device=DEV)
    K.gp_variance(7, specs, x, list(both[:, 2]), N=N, obs=dbs, y_out=list(both[:, 0]), w_out=list(both[:, 1]), grid=2)
    for b in range(2):
        K.gp_variance(7, specs[b], x, one[b, 2], N=N, obs=dbs[b], y_out=one[b, 0], w_out=one[b, 1], grid=2)
    assert torch.equal(both.view(torch.int32), one.view(torch.int32)) and (both[:, 1] > 0).any(1).all()
    assert not both[:, :, 64:128].any()          # DN16 nodata decodes to y = 0: (y, 0, var 0)


@pytest.mark.parametrize("layout", list(V.LAYOUTS))
def test_non_finite_pixel_fails_open_and_stays_contained(layout):
    N, bad = 513, 100
    c, db = V.case(layout, 33, N), W.band("f32mask", N, DEV)
    db.w[bad], db.mask[bad] = 2500.0, 1           # the pixel is observed
    clean = W.launch(c, db, N, DEV, grid=2)
    x = c["x"].copy()
    x[c["smap"][1], bad] = np.nan
    got = W.launch(c, db, N, DEV, x=x, grid=2)
    others = np.arange(N) != bad
    assert got[1, bad] == np.float32(2500.0) and np.isnan(got[2, bad]) and 0 < clean[1, bad] < 2500.0
    assert np.array_equal(got[:, others].view(np.int32), clean[:, others].view(np.int32))


def test_engine_inflate():
    kf, st = V.engine_run(DEV, emulator_uncertainty="inflate")
    N = st.N
    assert kf.last_emulator_std.shape == (2, N) and kf.last_emulator_std.is_cuda
    for (sp, db), (_, run) in zip(kf.last_inflate_source, kf.last_inflate_bands):
        y, w = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
        K.gp_variance(7, sp, kf.last_inflate_x, None, N=N, obs=db, y_out=y, w_out=w)
        assert run.kind == K.OBS_F32 and (w > 0).any()
        assert torch.equal(y.view(torch.int32), run.y[:N].view(torch.int32))
        assert torch.equal(w.view(torch.int32), run.w[:N].view(torch.int32))
    rec = [r for r in kf.metrics.records if r.get("event") == "date"][-1]["emulator"]
    assert len(rec) == 2 and all(r["max"] >= r["mean"] > 0 and 0 < r["weight_ratio"] < 1 for r in rec)
    (_, st0), (_, st1) = V.engine_run(DEV, emulator_uncertainty="off"), V.engine_run(DEV, emulator_uncertainty="report")
    assert torch.equal(st0.x, st1.x) and torch.equal(st0.P, st1.P)
    assert torch.isfinite(st.x[:, :N]).all() and not torch.equal(st.x, st0.x)
    for bad in (dict(innovation_gate=3.0), dict(band_sequential=True)):
        with pytest.raises(ValueError, match="inflate"):
            V.engine_run(DEV, emulator_uncertainty="inflate", **bad)
