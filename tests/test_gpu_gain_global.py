"""The gain (covariance) form on the matrix cores for 10-parameter states
(kf_device.h gain_mfma_g_kernel: every band's table read from global memory):
the kernel against the float64 oracle and against the VALU gain kernel, the
fused prior-reset forecast with line tables and the fused output, and the
Sentinel-2 configuration of the engine (SAIL prior reset, no propagator) with
nothing stored on the dates whose analysis nobody reads."""
from __future__ import annotations

import datetime as dt

import numpy as np
import pytest
import torch

import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.engine.bands import RecordCache, build_table
from kafka_inferenceengine_amd.inference import gain_blocks
from kafka_inferenceengine_amd.ops import kernels as K
from kafka_inferenceengine_amd.utils.blocks import ntri, pack_matrix, unpack_blocks

import kernel_cases as C
from test_oracles import dbands, oracle_bands, prosail_problem, x_err

pytestmark = pytest.mark.gpu


def _with_variant(variant, fn):
    old = K.DEFAULT_VARIANT
    K.DEFAULT_VARIANT = variant
    try:
        return fn()
    finally:
        K.DEFAULT_VARIANT = old


def _p_err(P_packed, Pr, n):
    d = np.sqrt(np.einsum("nii->ni", Pr))
    return float(np.max(np.abs(unpack_blocks(P_packed, n) - Pr) / (d[:, :, None] * d[:, None, :])))


def _clouded(N, n_bands, seed, n_train, dark):
    """prosail_problem (single bands masked at random) with every band of the
    pixels ``dark`` at weight 0."""
    prob = prosail_problem(N=N, n_bands=n_bands, seed=seed, n_train=n_train)
    for y, w in prob["obs"]:
        w[dark] = 0.0
    prob["bands"] = [(y.astype(np.float64), w.astype(np.float64)) for y, w in prob["obs"]]
    return prob


def _gain_launch(prob, dev):
    n, N = prob["n"], prob["N"]
    tab = build_table(prob["specs"], dbands(prob, dev), n, RecordCache(), dev)
    assert tab.gpm_global and tab.gpm_frags == 0 and tab.layout == K.BAND_LAYOUT_SHARED_X
    Pcov = np.linalg.inv(prob["Pf"])
    xo = torch.zeros((n, N), device=dev)
    po = torch.zeros((ntri(n), N), device=dev)
    st = torch.zeros(N, dtype=torch.uint8, device=dev)
    K.gain(n, tab, C.soa(prob["x"], dev), C.soa(prob["xf"], dev), C.packed(Pcov, dev), xo, po, st)
    torch.cuda.synchronize()
    return xo.cpu().numpy().T, po.cpu().numpy(), st.cpu().numpy()


# (a) ten bands: tail lanes, two waves without any observation, three 32-point
# chunks with the last one padded; (b) 13 + 21 bands: band table offsets and the
# per-band constant patch of the shared exponent operand
@pytest.mark.parametrize("n_bands,N,n_train,dark", [(10, 64 * 5 + 19, 70, slice(64, 192)),
                                                    (34, 64 * 3 + 5, 40, slice(64, 128))])
def test_gain_global_kernel_vs_float64_and_valu(cuda, n_bands, N, n_train, dark):
    prob = _clouded(N, n_bands, 41 + n_bands, n_train, dark)
    n = prob["n"]
    xm, pm, sm = _gain_launch(prob, cuda)
    xv, pv, sv = _with_variant(K.Variant.VALU_ORACLE, lambda: _gain_launch(prob, cuda))
    xp, pp, sp = _with_variant(K.Variant.PER_BAND_OPERAND, lambda: _gain_launch(prob, cuda))
    xr, Pr = gain_blocks(prob["x"], prob["xf"], np.linalg.inv(prob["Pf"]), oracle_bands(prob, prob["x"]))
    ex_m, ex_v = x_err(xm, xr), x_err(xv, xr)
    ep_m, ep_v = _p_err(pm, Pr, n), _p_err(pv, Pr, n)
    print(f"gain {n_bands} bands: x err mfma {ex_m:.2e} valu {ex_v:.2e}; P err mfma {ep_m:.2e} valu {ep_v:.2e}")
    assert ex_m < 1e-4 and ep_m < 2e-4, (ex_m, ep_m)
    assert np.array_equal(sm, sv)
    assert np.all(sm[dark] & K.ST_NO_OBS) and not np.any(np.delete(sm, np.r_[dark]) & K.ST_NO_OBS)
    assert not np.array_equal(xm, xv)          # the matrix-core kernel ran
    assert ex_m <= 1.5 * ex_v + 1e-5, (ex_m, ex_v)
    assert ep_m <= 1.5 * ep_v + 1e-5, (ep_m, ep_v)
    # the exponent operand built once per iteration or per band: the same bits
    assert np.array_equal(xm, xp) and np.array_equal(pm, pp) and np.array_equal(sm, sp)


def test_gain_global_prior_reset_line_tables_and_output(cuda):
    """The fused prior-reset forecast (PROP_PRIOR, nothing propagated) over an
    analysis covariance, GN 1 + 2 in one launch in the observed-first order,
    uncertainty raster from the kernel; the first iteration from the line
    tables (one point: every pixel is at the reset mean) or from the GP sums."""
    prob = prosail_problem(N=64 * 4 + 7, n_bands=10, seed=43, n_train=70)
    n, N = prob["n"], prob["N"]
    rng = np.random.default_rng(43)
    mu, _, Pi = k.sail_prior()
    spec = {"mode": 0, "m": np.ones(n), "q": np.zeros(n), "prop_mask": 0, "reset_mean": mu,
            "reset_cinv": pack_matrix(Pi), "blend": False}
    xa = C.soa(prob["x"], cuda)
    pa = C.packed(np.linalg.inv(C.spd_blocks(rng, N, n, 20.0)), cuda)     # analysis covariance (not read)
    mu32 = np.asarray(mu, dtype=np.float32).astype(np.float64)
    xf = np.broadcast_to(mu32, (N, n)).copy()
    Pf = np.broadcast_to(np.linalg.inv(Pi), (N, n, n)).copy()

    def launch(line, gn_fused):
        h0 = [torch.zeros(N, dtype=torch.float32, device=cuda) for _ in range(10)]
        tab = build_table(prob["specs"], dbands(prob, cuda), n, RecordCache(), cuda, h0)
        assert tab.gpm_global
        h = K.prop_args(n, spec, xa, pa, fused=True)
        if line:
            assert K.line_fields(tab, h, n, cuda) is not None
        order, _ = K.obs_order(tab, N, cuda)
        xo = torch.zeros((n, N), device=cuda)
        unc = torch.zeros((n, N), device=cuda)
        st = torch.zeros(N, dtype=torch.uint8, device=cuda)
        pf = torch.zeros(K.grid_for(N), dtype=torch.float64, device=cuda) if gn_fused == 2 else None
        K.gain(n, tab, None, None, None, xo, None, st, None, prop=h, out=(None, unc, None), gn_fused=gn_fused,
               partials_first=pf, order=order, line=line)
        torch.cuda.synchronize()
        return (xo.cpu().numpy().T, unc.cpu().numpy().T, [t.cpu().numpy().astype(np.float64) for t in h0],
                st.cpu().numpy())

    (x_on, u_on, _, s_on), (x_off, u_off, _, s_off) = launch(True, 2), launch(False, 2)
    assert np.array_equal(s_on, s_off) and not np.any(s_on & K.ST_FALLBACK)
    assert not np.array_equal(x_on, x_off)        # the line tables were used
    assert np.abs(x_on - x_off).max() < 2e-3, np.abs(x_on - x_off).max()
    # first-iteration H0 at the reset mean against the float64 emulators
    errs = {}
    for line in (True, False):
        h0 = launch(line, 1)[2]
        e = 0.0
        for b in range(10):
            sel = prob["bands"][b][1] > 0
            H, _ = prob["ems"][b].predict(xf)
            e = max(e, float(np.abs(h0[b][sel] - H[sel]).max()))
        errs[line] = e
    print(f"first-iteration H0 error: line {errs[True]:.2e}, GP sums {errs[False]:.2e}")
    assert errs[True] < 2e-6, errs
    assert errs[True] <= errs[False] + 1e-7, errs
    # two float64 iterations: the second linearised at the first's analysis
    x1, _ = gain_blocks(xf, xf, Pf, oracle_bands(prob, xf))
    x2, P2 = gain_blocks(x1, xf, Pf, oracle_bands(prob, x1))
    unc_r = 1.0 / np.sqrt(np.einsum("nii->ni", np.linalg.inv(P2)))
    for tag, x, u in (("line", x_on, u_on), ("sums", x_off, u_off)):
        ex, eu = x_err(x, x2), float(np.max(np.abs(u - unc_r) / unc_r))
        print(f"gain prior reset ({tag}): x {ex:.2e} unc {eu:.2e}")
        assert eu < 1e-4, (tag, eu)


DATES = [dt.datetime(2017, 7, 3) + dt.timedelta(days=5 * i) for i in range(4)]
GRID = [DATES[0] - dt.timedelta(days=1)] + [d + dt.timedelta(days=1) for d in DATES]


def _dist(a, b, floor=0.05):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float(((a - b).abs() / b.abs().amax(dim=-1, keepdim=True).clamp(min=floor)).max())


def test_gain_global_engine_s2_prior_reset(cuda, monkeypatch):
    """The reference's S2 configuration (10-parameter SAIL state, prior reset,
    covariance form) through the engine: the gain form on the device against
    the host runner of the same code and against the information form, the
    per-chunk Gauss-Newton counts, and the stored-rows policy -- no covariance
    row stored on the intermediate dates, the full one on the last."""
    mask = np.ones((64, 60), bool)
    mask[5:12, 3:30] = False
    stores = []
    real_gain = K.gain

    def spy(n_params, bands, x_prev, x_f, p_f, x_out, p_out=None, *a, **kw):
        stores.append((p_out is not None, int(kw.get("pdiag_rows", 0))))
        return real_gain(n_params, bands, x_prev, x_f, p_f, x_out, p_out, *a, **kw)

    monkeypatch.setattr(K, "gain", spy)

    def run(dev, **cfg):
        obs = k.SyntheticS2Observations(mask, dates=DATES, n_bands=10, n_train=64, device=dev, stream=False,
                                        n_pool=2, seed=3)
        prior = k.SAILPrior(k.SAIL_PARAMETERS, mask)
        out = k.DeviceOutput(k.SAIL_PARAMETERS)
        kf = k.LinearKalman(obs, out, mask, k.create_prosail_observation_operator, k.SAIL_PARAMETERS,
                            state_propagation=None, prior=prior, device=dev,
                            config=k.EngineConfig(convergence_chunk=[32, 32], store_precision="auto", **cfg))
        del stores[:]
        per_date = []
        real_do = kf.do_all_bands_state

        def do(*a, **kw):
            n0 = len(stores)
            res = real_do(*a, **kw)
            per_date.append((list(stores[n0:]), res.state.p_valid))
            return res

        kf.do_all_bands_state = do
        st = kf.run(GRID, kf.state_from_prior(prior), None, None)
        if torch.device(dev).type == "cuda":
            torch.cuda.synchronize()
        N = st.N
        return dict(st=st, x=st.x[:, :N].cpu(), unc=out.unc.cpu(), N=N, per_date=per_date, kf=kf,
                    gn=[h.get("gn_iterations") for h in kf.history], hist=[h.get("chunk_iters") for h in kf.history])

    info = run(cuda)
    gain = run(cuda, analysis_form="gain")
    host = run("cpu", analysis_form="gain")
    valu = _with_variant(K.Variant.VALU_ORACLE, lambda: run(cuda, analysis_form="gain"))
    assert info["gn"] == gain["gn"] == host["gn"]
    assert info["hist"] == gain["hist"] == host["hist"] and all(h is not None for h in gain["hist"])
    # the device against the host runner of the same gain code
    assert _dist(gain["x"], host["x"]) < 1e-3, _dist(gain["x"], host["x"])
    assert _dist(gain["unc"], host["unc"]) < 1e-3, _dist(gain["unc"], host["unc"])
    # against the information form: no further than the VALU gain kernel is
    for key in ("x", "unc"):
        dm, dv = _dist(gain[key], info[key]), _dist(valu[key], info[key])
        print(f"gain vs information form, {key}: matrix cores {dm:.2e}, VALU {dv:.2e}")
        assert dm <= 1.5 * dv + 1e-4, (key, dm, dv)
    # stored rows: nothing on the intermediate dates, the full covariance on the last
    for r in (gain, host):
        assert len(r["per_date"]) == len(DATES)
        for launches, p_valid in r["per_date"][:-1]:
            assert launches and all(not stored for stored, _ in launches), launches
            assert p_valid == 0
        launches, p_valid = r["per_date"][-1]
        assert p_valid is None and any(stored and rows == 0 for stored, rows in launches), launches
    st = gain["st"]
    st.require_full("the last date")
    P = unpack_blocks(st.P[:, :st.N].cpu().numpy(), 10).astype(np.float64)
    assert np.isfinite(P).all() and np.all(np.linalg.eigvalsh(P) > 0)
    # for the record only (no pin: the two runs' last linearisation points differ
    # by up to the 1e-3 above, and the covariance follows the Jacobian there)
    Ph = unpack_blocks(host["st"].P[:, :st.N].cpu().numpy(), 10).astype(np.float64)
    dh = np.sqrt(np.einsum("nii->ni", Ph))
    ep = float(np.max(np.abs(P - Ph) / (dh[:, :, None] * dh[:, None, :])))
    print(f"last date's covariance, device vs host runner: {ep:.2e}")
