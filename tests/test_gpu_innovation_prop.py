"""``K.innovation(prop=...)`` (csrc/kf_gp_mfma.h ``pixel_innovation_prop``) against the float64 oracle at the
float64 partial-reset forecast (``make_partial_prior_propagator``'s formulas, kept in float64) of the same float32
analysis: x_f,j = x_a,j (m = 1, exact), (P_f)_jj = 1 / (1 / (P_a)_jj + q), the reset mean and precision elsewhere.
The bound is test_gpu_innovation_mfma's plus the rounding of that entry, which the kernel forms as
rcp(rcp(pa) + q): two reciprocals of at most 1 ulp = 2 U and one addition of U, a relative error of (P_f)_jj of at
most 5 U, which moves s = h^T C h (C = P_f^-1) by at most 5 U (P_f)_jj (C h)_j^2.  The analysis rows the forecast
does not read hold NaN.  Measured err / bound: BENCHMARKS.md."""
import dataclasses
import json

import numpy as np
import pytest
import torch

import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.ops import kernels as K
from kafka_inferenceengine_amd.utils.blocks import pack_matrix

import kernel_cases as C
import test_innovation as TI
from test_evidence import compare
from test_engine import _grid
from test_gpu_innovation_mfma import truth
from test_innovation import NS, SENT, SENT8, U, near_gate, screened_like
from test_innovation_mfma import gp_table
from test_marginal import blocks_of, spd_blocks

pytestmark = pytest.mark.gpu
J, QJ = 6, 0.04      # the propagated parameter (TLAI / the seventh PROSAIL input) and its model error
_CASES = {}


def prop_case(state, N):
    if (state, N) not in _CASES:
        rng = np.random.default_rng([11, N, state == "tip"])
        if state == "tip":
            prob = C.tip_problem(N=4, seed=8, n_train=60)
            ems, specs, maps, (mu, _, Pi) = prob["ems"], prob["specs"], k.TIP_BAND_MAPPER, k.tip_prior()
            t, t_out = rng.uniform(0.1, 0.9, N), 1.8      # t_out: past the line table's range (models/gp.py line_range)
        else:
            ems = k.make_prosail_emulators(n_bands=5, n_train=40, seed=0)
            specs, maps = [k.gp_spec(em, range(10)) for em in ems], [list(range(10))] * 5
            lo, hi = np.min([em.inputs.min(0) for em in ems], 0), np.max([em.inputs.max(0) for em in ems], 0)
            mu, Pi = 0.5 * (lo + hi), spd_blocks(10, 1e2, 1, 5)[0]
            # no coupling of J: the forecast stays SPD whatever its propagated diagonal entry is
            Pi[J, :J], Pi[J, J + 1:], Pi[:J, J], Pi[J + 1:, J] = 0.0, 0.0, 0.0, 0.0
            t, t_out = lo[J] + (hi[J] - lo[J]) * rng.uniform(0.2, 0.8, N), hi[J] + 0.8 * (hi[J] - lo[J])
        n, nb, jj = len(mu), len(specs), K._tri(len(mu), J, J)
        mu, Pi = C.f32(mu), C.sym32(Pi[None])[0]
        xa, pa = np.full((N, n), np.nan), np.full((K.ntri(n), N), np.nan)
        xa[:, J], pa[jj] = C.f32(t), C.f32(rng.uniform(5.0, 50.0, N))
        xf, Pf = np.tile(mu, (N, 1)), np.tile(Pi, (N, 1, 1))
        xf[:, J], Pf[:, J, J] = xa[:, J], 1.0 / (1.0 / pa[jj] + float(C.f32(QJ)))
        cov = np.linalg.inv(Pf)
        H0, h = np.empty((nb, N)), np.zeros((nb, N, n))
        for b, (em, mp) in enumerate(zip(ems, maps)):
            H0[b], h[b][:, mp] = em.predict(xf[:, mp])
        w = C.f32(np.where(rng.random((nb, N)) < 0.2, 0.0, 2500.0))
        y = C.f32(H0 + 2.0 * rng.standard_normal((nb, N)) * np.sqrt(np.einsum("bpi,pij,bpj->bp", h, cov, h) + 4e-4))
        spec = {"mode": 1, "m": np.ones(n), "q": np.full(n, QJ), "prop_mask": 1 << J, "reset_mean": mu,
                "reset_cinv": pack_matrix(Pi)}
        _CASES[state, N] = dict(n=n, nb=nb, N=N, specs=specs, spec=spec, xa=xa, pa=pa, A=Pf, cov=cov, y=y, w=w, H0=H0,
                                h=h, kind="precision", t_out=t_out, r_scale=np.abs(H0) + np.abs(y),
                                family="innovation_prop_kernel" if state == "tip" else "innovation_prop_g_kernel")
    return dict(_CASES[state, N])


def launch(g, joint=False, line=None, screened=False, xa=None, pa=None, **kw):
    n, N, dev = g["n"], g["N"], "cuda"
    tab, obs = gp_table(g["specs"], n, dev, g["y"], g["w"])
    o = dict(z=torch.full((g["nb"], N), SENT, device=dev),
             **{key: torch.full((N,), SENT, device=dev) for key in ("chi2", "d2", "logdet")[:3 if joint else 1]},
             **{key: torch.full((N,), SENT8, dtype=torch.uint8, device=dev) for key in ("nobs", "nrej", "status")})
    scr = [t.to(dev) for t in screened_like(obs)] if screened else None
    x = C.soa(g["xa"] if xa is None else xa, dev)
    p = torch.tensor(g["pa"] if pa is None else pa, dtype=torch.float32, device=dev)
    K.innovation(n, tab, x, p, kind="precision", screened=scr, prop=K.prop_args(n, g["spec"], x, p, fused=True),
                 line=line, **o, **kw)
    assert (K.LAST_INNOVATION_PLAN["family"], K.LAST_INNOVATION_PLAN["joint"]) == (g["family"], joint)
    return dict({key: v.cpu().numpy() for key, v in o.items()}, obs=obs, screened=scr and [t.cpu() for t in scr])


@pytest.mark.parametrize("line", [False, True])
@pytest.mark.parametrize("joint", [False, True])
@pytest.mark.parametrize("state,N", [(s, N) for s in ("tip", "prosail") for N in NS])
def test_against_float64_at_the_float64_forecast(state, N, joint, line):
    g = prop_case(state, N)
    h, cov, pjj = g["h"], g["cov"], g["A"][:, J, J]
    z64, nobs64, _, counted, ph, bound = truth(g)      # test_gpu_innovation_mfma's oracle and bound ...
    ch = np.einsum("pij,bpj->bpi", cov, h)
    d = np.einsum("bpi,pij,bpj->bp", h, cov, h) + 1.0 / np.where(counted, g["w"], 1.0)
    # ... plus the forecast's term of the module docstring, an error of s: z_bound's |z| * 0.5 * e_s / (s + 1 / w)
    bound = bound + np.abs(np.nan_to_num(z64)) * 0.5 * 5.0 * U * pjj[None, :] * ch[:, :, J] ** 2 / d
    out = launch(g, joint, line)
    assert np.array_equal(np.isnan(out["z"]), ~counted)
    err = np.abs(np.where(counted, out["z"] - np.nan_to_num(z64), 0.0))
    print(f"{state} N={N} joint={joint} line={line}: z max err/bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    assert np.array_equal(out["nobs"], nobs64) and not out["status"].any() and not out["nrej"].any()
    own = np.sum(np.nan_to_num(out["z"].astype(np.float64)) ** 2, axis=0)
    assert np.all(np.abs(out["chi2"] - own) <= (g["nb"] + 1) * U * own)
    if joint:      # test_gpu_innovation_mfma's first-order terms of the operator tolerances, the forecast's with them
        ex_d, ex_l = np.zeros(N), np.zeros(N)
        for p in np.nonzero(counted.any(axis=0))[0]:
            sel = counted[:, p]
            hp, cj = h[sel, p], np.abs(ch[sel, p, J])
            Si = np.linalg.inv(hp @ cov[p] @ hp.T + np.diag(1.0 / g["w"][sel, p]))
            u = np.abs(Si @ (g["y"][sel, p] - g["H0"][sel, p]))
            dS = 5e-5 * (ph[sel, p][:, None] + ph[sel, p][None, :]) + 5.0 * U * pjj[p] * np.outer(cj, cj)
            ex_d[p], ex_l[p] = 2.0 * u.sum() * 5e-6 + u @ dS @ u, np.sum(np.abs(Si) * dS)
        compare(g, out, f"{state} N={N} line={line} prop", extra_d2=ex_d, extra_ld=ex_l)


@pytest.mark.parametrize("state", ["tip", "prosail"])
def test_line_fallback_and_containment(state):
    """N = 130: two full tiles and a tail.  Pixel 70's propagated parameter lies outside the line table, so wave 1
    runs the sums: the bits of the ``line=False`` launch.  Pixel 5's analysis makes the forecast non-SPD: it fails
    open.  Every other lane of waves 0 and 2 keeps the bits of the clean launch, which is all inside the table."""
    g = prop_case(state, 130)
    g["w"] = g["w"].copy()
    g["w"][:, [5, 70]] = 2500.0      # both observed in every band
    kw = dict(joint=True, screened=True, gate=1.0, scope="band")
    clean = launch(g, line=True, **kw)
    xa, pa = g["xa"].copy(), g["pa"].copy()
    xa[70, J], pa[K._tri(g["n"], J, J), 5] = g["t_out"], -1.0
    out, sums = launch(g, line=True, xa=xa, pa=pa, **kw), launch(g, line=False, xa=xa, pa=pa, **kw)
    wave1 = np.arange(130) // 64 == 1
    rest = ~wave1 & (np.arange(130) != 5)
    assert out["status"][5] == 1 and not out["nrej"][5] and not out["nobs"][5] and \
        all(np.isnan(out[key][..., 5]).all() for key in ("z", "chi2", "d2", "logdet"))
    assert out["status"][70] == 0 and out["nobs"][70] == g["nb"]
    for key in ("z", "chi2", "nobs", "nrej", "status", "d2", "logdet"):
        assert np.array_equal(out[key][..., wave1], sums[key][..., wave1], equal_nan=True), key
        assert np.array_equal(out[key][..., rest], clean[key][..., rest], equal_nan=True), key
    for a, b, c, o in zip(out["screened"], sums["screened"], clean["screened"], out["obs"]):
        assert torch.equal(a[wave1], b[wave1]) and torch.equal(a[rest], c[rest]) and a[5] == o.w.cpu()[5]
    # the sums differ from the cubics by rounding: the fallback shows in wave 1's other lanes
    assert not np.array_equal(out["z"][:, wave1], clean["z"][:, wave1], equal_nan=True)


SHAPE, GATE, PLANTED = (64, 66), 3.0, {1: 0.3, 2: 0.25}      # date index -> reflectance added on rows 20..27, cols 30..37


def engine(src, s, device, **cfg):
    """One run -> (final state, rasters, {date: rejects, forecast and bands of the check, analysis plan})."""
    out, rec = k.DeviceOutput(k.TIP_PARAMETERS, keep_history=True), {}
    kf = k.LinearKalman(src, out, s[0], k.create_nonlinear_observation_operator, k.TIP_PARAMETERS,
                        state_propagation=k.propagate_information_filter_LAI, device=device, config=k.EngineConfig(**cfg))
    kf.set_trajectory_model()
    kf.set_trajectory_uncertainty(s[5])
    screen, analyse = kf._screen_date, kf.do_all_bands_state

    def screened(step, bands, fc):
        fc, kept = screen(step, bands, fc)
        rec[step] = dict(rej=[(b0.w > 0) & (b1.w == 0) for (_, b0), (_, b1) in zip(bands, kept)], fc=fc, bands=bands,
                         choice=kf._innov_forecast)
        return fc, kept

    def analysed(step, *a, **kw):
        res = analyse(step, *a, **kw)
        rec.setdefault(step, {})["plan"] = K.LAST_PLAN and K.LAST_PLAN["name"]
        return res
    kf._screen_date, kf.do_all_bands_state = screened, analysed
    return kf.run(s[1], s[3], None, s[4]), out.history, rec


def engine_case(device, seed=5):
    mask = np.ones(SHAPE, bool)
    obs = k.SyntheticBHRObservations(mask, n_train=60, stream=False, n_pool=4, device=device, seed=seed, field_cell=8,
                                     encoding="f32", cloud_fraction=0.0)
    x0, Pinv = k.JRCPrior(k.TIP_PARAMETERS, mask).process_prior(None)
    Q = np.zeros_like(x0)
    Q[6::7] = 0.04
    patch = np.zeros(SHAPE, bool)
    patch[20:28, 30:38] = True
    patch, amp = torch.from_numpy(patch[mask]).to(device), {obs.dates[i]: a for i, a in PLANTED.items()}
    src = TI.EditedSource(obs, lambda date, bands: bands if date not in amp else [
        dataclasses.replace(db, y=torch.where(patch, db.y + amp[date], db.y)) for db in bands])
    return (mask, _grid(5), src, x0, Pinv, Q)


def oracle_near_gate(rec):
    """Per recorded date of a materialised run: the float64 rejects at GATE and the band-pixels within the bound of it."""
    res = {}
    for date, d in rec.items():
        N = d["fc"].x.shape[1]
        x, A = d["fc"].x.cpu().numpy().astype(np.float64).T, blocks_of(d["fc"].P.cpu().numpy(), 7, N)
        y, w = (np.stack([getattr(db, key).cpu().numpy().astype(np.float64) for _, db in d["bands"]]) for key in "yw")
        H0, h = np.empty((2, N)), np.zeros((2, N, 7))
        for b, (_, db) in enumerate(d["bands"]):
            H0[b], h[b][:, k.TIP_BAND_MAPPER[b]] = db.emulator.predict(x[:, k.TIP_BAND_MAPPER[b]])
        g = dict(n=7, A=A, cov=np.linalg.inv(A), y=y, w=w, H0=H0, h=h, kind="precision", r_scale=np.abs(H0) + np.abs(y))
        z64, _, rej64, _, _, bound = truth(g, gate=GATE, scope="group")
        res[date] = rej64, near_gate(g, z64, bound, GATE, "group", [0, 0])
    return res


def test_engine_fused_equals_the_ungated_run_on_its_own_rejects(tmp_path):
    """JRC-TIP, 64 x 66, 4 dates, planted outliers, gate 3.  The float64 oracle (at the materialised run's forecasts)
    leaves no band-pixel within the z bound of the gate, so 'fused' and 'materialised' must reject what it rejects;
    the fused run's state and rasters are the default ungated run's on the source edited by those rejects, and every
    screened date's analysis takes that run's kernel.  The fused run also asks for the evidence: its second,
    kept-bands launch takes the JOINT kernel at the fused forecast."""
    s = engine_case("cuda")
    cfg = dict(innovation_gate=GATE, innovation_gp="mfma")
    _, _, mat = engine(s[2], s, "cuda", **cfg)
    want = oracle_near_gate(mat)
    assert not any(near.any() for _, near in want.values()) and sum(int(r.sum()) for r, _ in want.values()) >= 256
    fa, fh, fused = engine(s[2], s, "cuda", innovation_forecast="fused", innovation_evidence=True,
                           metrics_path=str(tmp_path / "m.jsonl"), **cfg)
    lines = [json.loads(ln) for ln in open(tmp_path / "m.jsonl")]
    assert [r["innovation"]["forecast"] for r in lines if r.get("event") == "date"] == ["materialised"] + 3 * ["fused"]
    assert [d["choice"] for _, d in sorted(fused.items())] == ["materialised"] + 3 * ["fused"]
    assert K.LAST_INNOVATION_PLAN["name"] == "innovation_prop_kernel<7, 4, true>"
    assert all(np.isfinite(r["innovation"]["loglik"]) for r in lines if r.get("event") == "date")
    for date, (rej64, _) in want.items():
        for run in (mat, fused):
            assert np.array_equal(torch.stack(run[date]["rej"]).cpu().numpy(), rej64), date

    def edit(date, bands):
        return bands if date not in fused else [dataclasses.replace(db, w=torch.where(r, torch.zeros_like(db.w), db.w))
                                                for db, r in zip(bands, fused[date]["rej"])]
    pa, ph, plain = engine(TI.EditedSource(s[2], edit), s, "cuda")
    assert {t: d["plan"] for t, d in fused.items()} == {t: d["plan"] for t, d in plain.items()}
    TI.same_run((None, fa, fh), (None, pa, ph))
