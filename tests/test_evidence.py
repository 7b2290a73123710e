"""The joint innovation statistic d2 = r^T S^-1 r, log det S and the Gaussian
log evidence (``ops.kernels.innovation`` ``d2`` / ``logdet``, csrc/kf_core.h
``pixel_innovation<NP, true>``; ``LinearKalman.evidence``; ``cli run
--evidence-out / --q-scale / --scan-q``): the per-pixel code on the host runner
against the float64 oracle ``evidence_blocks``, identities, the failure rule,
JRC-TIP GP bands, and the engine's accumulators against the batch log density.

Truth is numpy float64 on the float32-rounded inputs: S = H C H^T + R over the
counted bands, d2 by ``solve``, log det S by ``slogdet`` -- the order-free
formula, not the kernel's recursion.  The kernel runs the sequential
scalar-band recursion (c = C v, s~ = v.c + 1/w, e = r - v.delta, d2 += e^2/s~,
logdet += log s~, delta += c e/s~, C -= c c^T/s~).  With u = 2^-24 the bound is

    e_J = (max(4 n kappa_s, 16) + 4 n nb kappa_R) u,
    |d2 - d2_64| <= e_J d2_64 + e_res,   |logdet - logdet_64| <= e_J + e_log:

* max(4 n kappa_s, 16) u is the project's factor-and-substitute bound
  (tests/test_marginal.py, tests/test_innovation.py): the relative error of
  v_b = U^-T h_b (precision rows) or of P h_b (covariance rows), hence of every
  entry of S - R, kappa_s the condition number of the block scaled to unit
  diagonal;
* each of the nb downdates C -= c c^T / s~ is n^2 fused operations whose
  rounding, relative to the entries of C, is n u; what a later band sees of it
  is an error of v^T C v relative to v^T C_0 v, while the quantity that enters
  d2 and logdet is s~ = v^T C v + 1/w_b, which the downdates have shrunk from
  v^T C_0 v + 1/w_b towards 1/w_b: the amplification is at most
  (v^T C_0 v + 1/w) / (1/w) <= lambda_max(R^-1/2 S R^-1/2) = kappa_R, the
  conditioning of S in noise units.  symv, the dot products, the reciprocal and
  the update of delta add the same order per band: 4 n nb kappa_R u in all.
  A relative error eps of every s~ is a relative error eps of each term of d2
  (a sum of non-negative terms) and an absolute error eps per band of logdet.

* e_res = 2 sum_b |(S^-1 r)_b| e_r,b is the residual's own rounding, the term
  a derivation of the recursion alone leaves out: r_b = y_b - H_b(x) is formed
  in float32 from n fused multiply-adds and a subtraction, an absolute error
  e_r,b = (n + 2) u (|offset| + sum |h_j x_j| + |y_b|) (the e_r of
  tests/test_innovation.py), and d(r^T S^-1 r) = 2 (S^-1 r) . dr.  Relative to
  d2 it is unbounded where a residual is small against its operands (the first
  pixel found: |r| = 0.015 of operands 0.52, e_J = 24 u, an error of 1.1 e_J
  d2 of which the recursion has no part: with nb = 1 it is the error of z^2
  too).  It does not touch logdet.
* e_log = (nb + 2) u sum_b |log s~_b| is the logarithm's own rounding, the other
  term left out: e_J bounds the error of the s~, an absolute error of each
  log s~ that does not grow with |log s~|, but the float32 logarithm is good to
  1 ulp of its result (2 u |log s~_b|; the device library's documented error,
  half that on the host) and each of the nb additions into logdet rounds the
  partial sum (u sum_{c <= b} |log s~_c|).  The blocks of these cases carry
  per-parameter units exp(+-3), so |log s~| reaches 10 and one ulp of it is
  16 u, against e_J = 20 u for n = nb = 1 (the device first exceeded e_J
  there, by 1.23).  The s~_b are the squared diagonal of the Cholesky factor of
  S in band order.

The identities with nb = 1 and with P-orthogonal rows hold to rounding alone;
their few-u tolerances are derived where they are asserted."""
import dataclasses
import datetime as dt
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.engine.bands import DeviceBand, RecordCache, build_table
from kafka_inferenceengine_amd.inference import evidence_blocks, innovation_blocks
from kafka_inferenceengine_amd.models.operators import _linear_device_spec
from kafka_inferenceengine_amd.ops import kernels as K

import kernel_cases as C
from test_engine import _engine
from test_innovation import (NS, SENT, SENT8, EditedSource, NODATA, PLANE, bits, engine_run, engine_setup, kappa_scaled,
                             linear_case, on_device, same_run, screened_like, tip_case, unfused_cfg)
from test_marginal import SIZES, U, blocks_of, pack_rows
from test_smoother import (_free_port, _grid, batch_posterior, chain_bound, cov_blocks, load_filtered, mask_with_holes)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG2PI = np.log(2.0 * np.pi)
NBS = (1, 2, 10, 34)


def run_joint(case, device="cpu", joint=True, gate=0.0, scope="group", groups=None, screened=False, x=None, p=None,
              obs=None):
    """One launch over sentinel-filled outputs, with (``joint``) or without d2 / logdet."""
    n, nb, N, ld = case["n"], case["nb"], case["N"], case["ld"]
    obs = on_device(case["obs"] if obs is None else obs, device)
    tab = build_table(case["specs"], obs, n, RecordCache(), device)
    z = torch.full((nb, ld), SENT, dtype=torch.float32, device=device)
    chi2, d2, logdet = (torch.full((ld,), SENT, dtype=torch.float32, device=device) for _ in range(3))
    nobs, nrej, status = (torch.full((ld,), SENT8, dtype=torch.uint8, device=device) for _ in range(3))
    scr = [t.to(device) for t in screened_like(obs)] if screened else None
    extra = dict(d2=d2, logdet=logdet) if joint else {}
    K.innovation(n, tab, (case["x"] if x is None else x).to(device), (case["p"] if p is None else p).to(device),
                 kind=case["kind"], N=N, z=z, chi2=chi2, nobs=nobs, nrej=nrej, status=status, gate=gate, scope=scope,
                 groups=groups, screened=scr, **extra)
    return dict(z=z.cpu().numpy(), chi2=chi2.cpu().numpy(), nobs=nobs.cpu().numpy(), nrej=nrej.cpu().numpy(),
                status=status.cpu().numpy(), d2=d2.cpu().numpy(), logdet=logdet.cpu().numpy(),
                screened=None if scr is None else [t.cpu() for t in scr])


def joint_truth(case, ok=None):
    return evidence_blocks(case["A"], case["y"], case["w"], case["H0"], case["h"], kind=case["kind"], ok=ok)


def counted_of(case):
    return ~np.isnan(innovation_blocks(case["A"], case["y"], case["w"], case["H0"], case["h"], kind=case["kind"])[0])


def kappa_r(case, counted):
    """lambda_max(R^-1/2 S R^-1/2) over each pixel's counted bands, [N] (1 where none is counted)."""
    N = case["N"]
    out = np.ones(N)
    for p in range(N):
        sel = counted[:, p]
        if sel.any():
            g = case["h"][sel, p] * np.sqrt(case["w"][sel, p])[:, None]
            out[p] = 1.0 + np.linalg.eigvalsh(g @ case["cov"][p] @ g.T)[-1]
    return out


def e_joint(case, counted):
    """The module docstring's e_J per pixel."""
    n, nb = case["n"], case["nb"]
    return (np.maximum(4.0 * n * kappa_scaled(case["A"]), 16.0) + 4.0 * n * nb * kappa_r(case, counted)) * U


def e_residual(case, counted):
    """The module docstring's e_res per pixel."""
    n, N = case["n"], case["N"]
    out = np.zeros(N)
    for p in range(N):
        sel = counted[:, p]
        if sel.any():
            Hp = case["h"][sel, p]
            S = Hp @ case["cov"][p] @ Hp.T + np.diag(1.0 / case["w"][sel, p])
            u = np.linalg.solve(S, case["y"][sel, p] - case["H0"][sel, p])
            out[p] = 2.0 * np.sum(np.abs(u) * (n + 2) * U * case["r_scale"][sel, p])
    return out


def e_log(case, counted):
    """The module docstring's e_log per pixel."""
    N = case["N"]
    out = np.zeros(N)
    for p in range(N):
        sel = counted[:, p]
        if sel.any():
            Hp = case["h"][sel, p]
            S = Hp @ case["cov"][p] @ Hp.T + np.diag(1.0 / case["w"][sel, p])
            out[p] = (sel.sum() + 2) * U * np.sum(np.abs(2.0 * np.log(np.diag(np.linalg.cholesky(S)))))
    return out


def compare(case, out, label, scale=1.0, extra_d2=0.0, extra_ld=0.0):
    """d2 / logdet of a launch against the oracle within scale * (e_J, e_res) (+ extras); returns the largest
    err / bound."""
    N = case["N"]
    d64, l64, nobs64, _ = joint_truth(case)
    counted = counted_of(case)
    eJ = scale * e_joint(case, counted)
    extra_d2 = extra_d2 + scale * e_residual(case, counted)
    extra_ld = extra_ld + scale * e_log(case, counted)
    d2, ld = out["d2"][:N].astype(np.float64), out["logdet"][:N].astype(np.float64)
    assert np.isfinite(d2).all() and np.isfinite(ld).all() and np.all(d2 >= 0.0)
    assert np.array_equal(out["nobs"][:N], nobs64) and np.all(out["status"][:N] == 0)
    none = nobs64 == 0
    assert np.all(d2[none] == 0.0) and np.all(ld[none] == 0.0)
    bd, bl = eJ * d64 + extra_d2, eJ + extra_ld
    ed, el = np.abs(d2 - d64), np.abs(ld - l64)
    some = ~none
    rd = float(np.max(ed[some] / bd[some])) if some.any() else 0.0
    rl = float(np.max(el[some] / bl[some])) if some.any() else 0.0
    print(f"{label}: d2 max err/bound {rd:.3f}, logdet max err/bound {rl:.3f}, counted {counted.mean():.2f}")
    assert np.all(ed <= bd) and np.all(el <= bl)
    assert np.all(out["d2"][N:] == SENT) and np.all(out["logdet"][N:] == SENT)
    return max(rd, rl)


def check_joint_linear(n, nb, N, kind, seed, device="cpu"):
    case = linear_case(n, nb, N, kind, seed)
    out = run_joint(case, device)
    compare(case, out, f"n={n} nb={nb} N={N} {kind} {device}")
    return case, out


@pytest.mark.parametrize("kind", K.MARGINAL_KINDS)
@pytest.mark.parametrize("nb", NBS)
@pytest.mark.parametrize("n", SIZES)
def test_joint_against_float64(n, nb, kind):
    for i, N in enumerate(NS):
        check_joint_linear(n, nb, N, kind, seed=100 * n + nb + i)


def high_snr_case(n, nb, N, kind, seed):
    """``linear_case`` with the observation variance drawn log-uniformly between
    1e-4 and 10 times the predicted variance h^T P h."""
    case = linear_case(n, nb, N, kind, seed)
    rng = np.random.default_rng([seed, 77])
    obs, y_all, w_all = [], [], []
    for b in range(nb):
        s = np.einsum("pi,pij,pj->p", case["h"][b], case["cov"], case["h"][b])
        sigma = np.sqrt(s * np.exp(rng.uniform(np.log(1e-4), np.log(10.0), N)))
        y = case["H0"][b] + 2.0 * rng.standard_normal(N) * np.sqrt(s + sigma ** 2)
        raw = C.encode_band(K.OBS_F32, y, sigma, rng, edges=False, band=b, nb=nb)
        obs.append(C.device_band(K.OBS_F32, raw, case["ld"], "cpu"))
        yd, wd = C.decode_model(K.OBS_F32, raw)
        y_all.append(yd), w_all.append(wd)
    return dict(case, obs=obs, y=np.stack(y_all), w=np.stack(w_all))


def check_high_snr(n, nb, kind, device="cpu", N=785):
    case = high_snr_case(n, nb, N, kind, seed=9 + n)
    counted = counted_of(case)
    ratio = 1.0 / (case["w"][counted] * np.einsum("bpi,pij,bpj->bp", case["h"], case["cov"], case["h"])[counted])
    assert ratio.min() < 2e-4
    compare(case, run_joint(case, device), f"high SNR n={n} nb={nb} {kind} {device} (kappa_R up to "
            f"{kappa_r(case, counted).max():.0f})")


@pytest.mark.parametrize("kind", K.MARGINAL_KINDS)
@pytest.mark.parametrize("n,nb", [(1, 2), (3, 10), (7, 2), (10, 34)])
def test_joint_high_signal_to_noise(n, nb, kind):
    check_high_snr(n, nb, kind)


@pytest.mark.parametrize("kind", K.MARGINAL_KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_single_band_d2_is_z_squared(n, kind):
    """nb = 1: s~ is the s + 1/w of z, bit for bit (the same operations in the
    same order), so d2 = e (e / s~) and z^2 = (e rsqrt(s~))^2 differ by their
    own roundings: the reciprocal, two products (3 u; the hardware reciprocal is
    1 ulp: 4 u) against the root, the quotient and the product (3 u, doubled by
    the square: 6 u): 10 u."""
    for N in NS:
        case = linear_case(n, 1, N, kind, seed=5 * n + N)
        out = run_joint(case)
        z = out["z"][0, :N].astype(np.float64)
        cnt = ~np.isnan(z)
        z2 = np.where(cnt, z, 0.0) ** 2
        assert np.all(np.abs(out["d2"][:N] - z2) <= 10 * U * z2)
        assert np.all(out["d2"][:N][~cnt] == 0.0) and np.all(out["logdet"][:N][~cnt] == 0.0)
        assert (~cnt).any() or N == 1


@pytest.mark.parametrize("kind", K.MARGINAL_KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_single_band_logdet_is_log_of_the_innovation_variance(n, kind):
    """nb = 1 with numbers float32 holds exactly: a diagonal block of powers of
    4, a Jacobian row with one power of 2, w a power of 2 -- the factor, v, s
    and s + 1/w are then exact, and logdet is the float32 logarithm of
    s + 1/w: 1 ulp of the result (2 u |log|) and its rounding, 4 u max(|log|, 1)."""
    rng = np.random.default_rng(n)
    N, ld = 257, 260
    kd = rng.integers(-2, 3, (N, n))
    blocks = np.zeros((N, n, n))
    blocks[:, np.arange(n), np.arange(n)] = 4.0 ** (kd if kind == "covariance" else -kd)
    j = int(rng.integers(0, n))
    coef = np.zeros(n)
    coef[j] = 0.5
    x = np.full((n, ld), np.nan, dtype=np.float32)
    x[:, :N] = rng.uniform(0.25, 0.75, (n, N))
    q = rng.integers(-3, 4, N)
    y = np.full(ld, 0.3, dtype=np.float32)
    w = np.zeros(ld, dtype=np.float32)
    w[:N] = 2.0 ** q
    case = dict(n=n, nb=1, N=N, ld=ld, kind=kind, x=torch.from_numpy(x), p=torch.from_numpy(pack_rows(blocks, ld)),
                specs=[_linear_device_spec(n, k.LinearOperator(coef, 0.125), None, 0)],
                obs=[DeviceBand(K.OBS_F32, y=torch.from_numpy(y), w=torch.from_numpy(w))])
    out = run_joint(case)
    st = 0.25 * 4.0 ** kd[:, j] + 2.0 ** -q
    want = np.log(st)
    assert np.all(out["nobs"][:N] == 1)
    assert np.all(np.abs(out["logdet"][:N] - want) <= 4 * U * np.maximum(np.abs(want), 1.0))


@pytest.mark.parametrize("kind", K.MARGINAL_KINDS)
@pytest.mark.parametrize("n", [2, 3, 4, 7, 10])
def test_orthogonal_rows_d2_is_chi2(n, kind):
    """Band b reads parameter b alone and the block is diagonal: the whitened
    rows are orthogonal exactly, every c has one entry, no downdate touches what
    a later band reads and v . delta is 0, so d2 = sum e^2 / s~ with the s~ of
    the z's: 10 u per term (the nb = 1 identity) and one rounding per
    addition in each of the two sums, (10 + 2 nb) u."""
    rng = np.random.default_rng(20 + n)
    N, ld, nb = 321, 324, n
    blocks = np.zeros((N, n, n))
    blocks[:, np.arange(n), np.arange(n)] = np.exp(rng.uniform(-3.0, 3.0, (N, n)))
    x = np.full((n, ld), np.nan, dtype=np.float32)
    x[:, :N] = rng.uniform(0.25, 0.75, (n, N))
    specs, obs = [], []
    for b in range(nb):
        coef = np.zeros(n)
        coef[b] = rng.uniform(0.2, 2.0)
        specs.append(_linear_device_spec(n, k.LinearOperator(coef, 0.05), None, 0))
        y = np.full(ld, 0.0, dtype=np.float32)
        y[:N] = rng.uniform(-1.0, 2.0, N)
        w = np.zeros(ld, dtype=np.float32)
        w[:N] = np.where(rng.random(N) < 0.8, np.exp(rng.uniform(-2.0, 6.0, N)), 0.0)
        obs.append(DeviceBand(K.OBS_F32, y=torch.from_numpy(y), w=torch.from_numpy(w)))
    case = dict(n=n, nb=nb, N=N, ld=ld, kind=kind, x=torch.from_numpy(x), p=torch.from_numpy(pack_rows(blocks, ld)),
                specs=specs, obs=obs)
    out = run_joint(case)
    chi2 = out["chi2"][:N].astype(np.float64)
    assert np.all(out["status"][:N] == 0) and out["nobs"][:N].max() == nb
    assert np.all(np.abs(out["d2"][:N] - chi2) <= (10 + 2 * nb) * U * chi2)


@pytest.mark.parametrize("kind", K.MARGINAL_KINDS)
def test_existing_outputs_unmoved(kind):
    """With and without d2 / logdet: z, chi2, nobs, nrej, status and the screened planes bit for bit."""
    for n, nb, N in ((1, 1, 65), (3, 5, 785), (7, 2, 785), (10, 34, 257)):
        case = linear_case(n, nb, N, kind, seed=31 + n)
        groups = [b % 3 for b in range(nb)]
        a = run_joint(case, joint=True, gate=2.0, scope="group", groups=groups, screened=True)
        b = run_joint(case, joint=False, gate=2.0, scope="group", groups=groups, screened=True)
        for key in ("z", "chi2"):
            assert np.array_equal(a[key].view(np.int32), b[key].view(np.int32)), key
        for key in ("nobs", "nrej", "status"):
            assert np.array_equal(a[key], b[key]), key
        for s, t in zip(a["screened"], b["screened"]):
            assert torch.equal(bits(s), bits(t))
        assert int(a["nrej"][:N].sum()) > 0 or N < 100
        # the launch without them leaves d2 / logdet alone
        assert np.all(b["d2"] == SENT) and np.all(b["logdet"] == SENT)


def check_joint_failure_rule(n, N, kind, device="cpu"):
    """Unscreenable pixels (block -I, NaN in the block, NaN in the state) and a
    step variance that is not finite (1 / w overflows) give NaN in both
    outputs; the neighbours equal the clean run bit for bit; tails untouched."""
    case = linear_case(n, 3, N, kind, seed=40 + n)
    clean = run_joint(case, device)
    iu = np.triu_indices(n)
    diag_rows = np.nonzero(iu[0] == iu[1])[0]
    pix = sorted({0, N // 2, N - 1})
    for bad, what in zip(pix, ("minus_identity", "nan_block", "nan_state")):
        x, p = case["x"].clone(), case["p"].clone()
        if what == "minus_identity":
            p[:, bad] = 0.0
            p[diag_rows, bad] = -1.0
        elif what == "nan_block":
            p[p.shape[0] - 1, bad] = float("nan")
        else:
            x[n - 1, bad] = float("nan")
        out = run_joint(case, device, x=x, p=p)
        assert out["status"][bad] == 1 and np.isnan(out["d2"][bad]) and np.isnan(out["logdet"][bad]), what
        keep = np.arange(N) != bad
        for key in ("d2", "logdet", "chi2", "nobs", "status"):
            assert np.array_equal(out[key][:N][keep], clean[key][:N][keep], equal_nan=True), (what, key)
        assert np.all(out["d2"][N:] == SENT) and np.all(out["logdet"][N:] == SENT)
    # 1 / w = inf: z = 0 is finite and counted, the step variance is not
    bad = N // 3
    obs = [dataclasses.replace(o, w=o.w.clone()) for o in case["obs"]]
    obs[1].w[bad] = 1e-45
    out = run_joint(case, device, obs=obs)
    assert out["status"][bad] == 0 and out["z"][1, bad] == 0.0 and np.isfinite(out["chi2"][bad])
    assert np.isnan(out["d2"][bad]) and np.isnan(out["logdet"][bad])
    keep = np.arange(N) != bad
    for key in ("d2", "logdet"):
        assert np.array_equal(out[key][:N][keep], clean[key][:N][keep]), key


@pytest.mark.parametrize("kind", K.MARGINAL_KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_joint_failure_rule(n, kind):
    check_joint_failure_rule(n, 65, kind)


def check_joint_gp(kind, device="cpu", N=785):
    """GP bands against float64 ``predict``.  The operator tolerances of
    test_kernels.py (H0 5e-6, h 5e-5 per entry, absolute) to first order, with
    u = S^-1 r and dS_bc = 5e-5 (sum_i |(P h_b)_i| + sum_i |(P h_c)_i|) the
    bound on an entry of S: d(d2) = 2 u . dr - u^T dS u, so d2 gains
    2 |u| . (5e-6) + |u|^T dS |u|; d(logdet) = tr(S^-1 dS), so logdet gains
    sum_bc |S^-1_bc| dS_bc."""
    prob, x32, ob = tip_case(N)
    Pf = C.sym32(prob["Pf"])
    blocks = Pf if kind == "precision" else C.sym32(np.linalg.inv(prob["Pf"]))
    cov = np.linalg.inv(blocks) if kind == "precision" else blocks
    y = np.stack([C.f32(r["y"]) for r in prob["raw"]])
    w = np.stack([C.f32(r["w"]) for r in prob["raw"]])
    H0 = np.stack([o[0] for o in ob])
    h = np.stack([o[1] for o in ob])
    case = dict(n=7, nb=2, N=N, kind=kind, A=blocks, cov=cov, y=y, w=w, H0=H0, h=h, r_scale=np.abs(H0) + np.abs(y))
    tab = C.table(prob, device)
    d2, logdet = (torch.full((N,), SENT, device=device) for _ in range(2))
    nobs, status = (torch.zeros(N, dtype=torch.uint8, device=device) for _ in range(2))
    K.innovation(7, tab, C.soa(x32, device), C.packed(blocks, device), kind=kind, nobs=nobs, status=status, d2=d2,
                 logdet=logdet)
    counted = counted_of(case)
    ph = np.abs(np.einsum("pij,bpj->bpi", cov, h)).sum(axis=2)
    ex_d, ex_l = np.zeros(N), np.zeros(N)
    for p in range(N):
        sel = counted[:, p]
        if not sel.any():
            continue
        Hp = h[sel, p]
        Si = np.linalg.inv(Hp @ cov[p] @ Hp.T + np.diag(1.0 / w[sel, p]))
        u = np.abs(Si @ (y[sel, p] - H0[sel, p]))
        dS = 5e-5 * (ph[sel, p][:, None] + ph[sel, p][None, :])
        ex_d[p] = 2.0 * u.sum() * 5e-6 + u @ dS @ u
        ex_l[p] = np.sum(np.abs(Si) * dS)
    out = dict(d2=np.append(d2.cpu().numpy(), SENT), logdet=np.append(logdet.cpu().numpy(), SENT),
               nobs=nobs.cpu().numpy(), status=status.cpu().numpy())
    assert counted.mean() > 0.5
    compare(case, out, f"tip GP {kind} {device}", extra_d2=ex_d, extra_ld=ex_l)


@pytest.mark.parametrize("kind", K.MARGINAL_KINDS)
def test_joint_tip_gp_bands_against_float64_predict(kind):
    check_joint_gp(kind)


def test_wrapper_refusals_of_the_joint_outputs():
    case = linear_case(3, 2, 20, "precision", seed=1)
    n, N, ld = 3, 20, case["ld"]
    tab = build_table(case["specs"], case["obs"], n, RecordCache(), "cpu")
    kw = dict(kind="precision", N=N, status=torch.zeros(ld, dtype=torch.uint8))
    K.innovation(n, tab, case["x"], case["p"], d2=torch.zeros(ld), **kw)          # either one alone
    K.innovation(n, tab, case["x"], case["p"], logdet=torch.zeros(N), **kw)
    with pytest.raises(ValueError, match="d2"):
        K.innovation(n, tab, case["x"], case["p"], d2=torch.zeros(N - 1), **kw)
    with pytest.raises(ValueError, match="logdet"):
        K.innovation(n, tab, case["x"], case["p"], logdet=torch.zeros(ld, dtype=torch.float64), **kw)


# ---------------------------------------------------------------- engine
def identity_case(x, blocks, kind, y, w):
    """The joint-statistic case of one date of identity observations (band b
    reads parameter b) against a state: x [N, n], blocks [N, n, n], y / w [n, N]."""
    N, n = x.shape
    cov = np.linalg.inv(blocks) if kind == "precision" else blocks
    return dict(n=n, nb=n, N=N, kind=kind, A=blocks, cov=cov, y=y, w=w, H0=x.T.copy(),
                h=np.broadcast_to(np.eye(n)[:, None, :], (n, N, n)).copy(), r_scale=np.abs(x.T) + np.abs(y))


def loglik_bound(case):
    """The kernel bound on one date's log evidence per pixel, (e_J d2 + e_res + e_J + e_log) / 2, and the
    oracle's values."""
    d64, l64, nobs, ll = joint_truth(case)
    counted = counted_of(case)
    eJ = e_joint(case, counted)
    return (np.where(nobs > 0, 0.5 * (eJ * d64 + e_residual(case, counted) + eJ + e_log(case, counted)), 0.0),
            (d64, l64, nobs, ll))


def state_error_term(case, ex, eP):
    """First-order effect on one date's log evidence of a forecast that is off
    by |dx_i| <= ex max_j |x_j| and |dP_ij| <= eP sqrt(P_ii P_jj) (the measures
    of tests/test_smoother.py), identity observations: with S = P[obs, obs] + R
    and u = S^-1 r, d(d2) = -2 u . dx - u^T dP u and d(logdet) = tr(S^-1 dP)."""
    N = case["N"]
    out = np.zeros(N)
    counted = counted_of(case)
    xs = np.abs(case["H0"]).max(axis=0)
    for p in range(N):
        sel = counted[:, p]
        if not sel.any():
            continue
        P = case["cov"][p][np.ix_(sel, sel)]
        Si = np.linalg.inv(P + np.diag(1.0 / case["w"][sel, p]))
        u = np.abs(Si @ (case["y"][sel, p] - case["H0"][sel, p]))
        d = np.sqrt(np.diag(P))
        dP = eP * d[:, None] * d[None, :]
        out[p] = 0.5 * (2.0 * u.sum() * ex * xs[p] + u @ dP @ u + np.sum(np.abs(Si) * dP))
    return out


def batch_log_density(x0, L0, W, Y, m, q):
    """Float64 log density per pixel of the stacked identity observations of T
    steps: with the matrices of ``test_smoother.batch_posterior`` (A, b) and A0
    the same matrix without the observation terms,
    -1/2 [sum w y^2 + x0^T L0 x0 - b^T A^-1 b] - 1/2 [log det A - log det A0 - sum log w] - (m / 2) log 2 pi."""
    T, N, n = W.shape
    q = np.broadcast_to(np.asarray(q, dtype=np.float64), (N, n))
    m = np.asarray(m, dtype=np.float64)
    A0 = np.zeros((N, T * n, T * n))
    b = np.zeros((N, T * n))
    A0[:, :n, :n] += L0
    b[:, :n] += np.einsum("pij,pj->pi", L0, x0)
    ar = np.arange(n)
    for t in range(T):
        s = t * n
        b[:, s:s + n] += W[t] * Y[t]
        if t + 1 < T:
            qi = 1.0 / q
            A0[:, s + ar, s + ar] += m * qi * m
            A0[:, s + n + ar, s + n + ar] += qi
            A0[:, s + ar, s + n + ar] -= m * qi
            A0[:, s + n + ar, s + ar] -= m * qi
    A = A0.copy()
    for t in range(T):
        A[:, t * n + ar, t * n + ar] += W[t]
    quad = np.sum(W * Y * Y, axis=(0, 2)) + np.einsum("pi,pij,pj->p", x0, L0, x0) \
        - np.einsum("pi,pi->p", b, np.linalg.solve(A, b[:, :, None])[:, :, 0])
    obs = W > 0
    logw = np.sum(np.log(np.where(obs, W, 1.0)), axis=(0, 2))
    return -0.5 * quad - 0.5 * (np.linalg.slogdet(A)[1] - np.linalg.slogdet(A0)[1] - logw) \
        - 0.5 * obs.sum(axis=(0, 2)) * LOG2PI


def record_forecasts(kf):
    """Wrap the engine's date check: {date: (x, P, kind, bands)} of every forecast it screens."""
    rec = {}
    inner = kf._screen_date

    def screen(step, bands, forecast):
        fc, run_bands = inner(step, bands, forecast)
        rec[step] = (fc.x.clone(), fc.P.clone(), fc.kind, run_bands)
        return fc, run_bands
    kf._screen_date = screen
    return rec


def check_engine_prediction_error_decomposition(tmp_path, form, device="cpu", T=5):
    """The linear identity-observation problem of test_smoother.check_engine_against_batch
    (exact propagator of the form, identity trajectory model): the run's
    per-pixel log evidence against the float64 batch log density of the
    stacked observations.

    Tolerance per pixel: the sum over the dates of the kernel bound on a
    date's log evidence, (e_J d2 + e_res + e_J + e_log) / 2 on the recorded forecast,
    plus the first-order effect (``state_error_term``) of a forecast off by
    T times the per-step state error of ``chain_bound``.  A pixel without an
    observation on any date has log evidence 0 and tolerance 0 but for the
    float64 floor below."""
    mask = mask_with_holes((24, 20))
    grid = _grid(T + 1)
    dates = [g + dt.timedelta(days=1) for g in grid[:T]]
    obs = k.SyntheticIdentityObservations(mask, dates=dates, device=device, stream=False, n_pool=T, field_cell=8,
                                          encoding="f32", cloud_fraction=0.35, seed=4)
    prior = k.JRCPrior(k.TIP_PARAMETERS, mask)
    x0, Pinv = prior.process_prior(None)
    n = 7
    q = 0.05 * np.diag(np.linalg.inv(np.asarray(prior.device_prior(None).cinv, dtype=np.float64)))
    q64 = q.astype(np.float32).astype(np.float64)
    prop = k.propagate_standard_kalman if form == "gain" else k.propagate_information_filter_SLOW
    kf = k.LinearKalman(obs, None, mask, k.create_linear_observation_operator, k.TIP_PARAMETERS,
                        state_propagation=prop, device=device,
                        config=k.EngineConfig(analysis_form=form, checkpoint_dir=str(tmp_path / "ck"),
                                              checkpoint_every=1, innovation_evidence=True))
    kf.set_trajectory_model()
    kf.set_trajectory_uncertainty(q)
    rec = record_forecasts(kf)
    kf.run(grid, x0, None, Pinv)
    N = kf.N
    assert sorted(rec) == dates and set(kf.last_innovation) == {"chi2", "nobs", "nrej", "status", "d2", "logdet"}
    W = np.zeros((T, N, n))
    Y = np.zeros((T, N, n))
    for t, d in enumerate(dates):
        for b in range(n):
            y, w = obs.get_device_band_data(d, b).decode()
            Y[t, :, b], W[t, :, b] = y.cpu().numpy()[:N], w.cpu().numpy()[:N]
    x0b, P0 = cov_blocks(kf.initial_state(x0, None, Pinv))
    want = batch_log_density(x0b, np.linalg.inv(P0), W, Y, np.ones(n), q64)
    filt = load_filtered(kf, tmp_path / "ck")
    _, bx, bP = chain_bound(filt, (1 << n) - 1, np.ones(n), q64, n)
    tol = np.zeros(N)
    dof = np.zeros(N, dtype=np.int64)
    per_date = np.zeros(N)
    for t, d in enumerate(dates):
        x, P, kind, _ = rec[d]
        case = identity_case(x.cpu().numpy()[:, :N].T.astype(np.float64), blocks_of(P.cpu().numpy(), n, N), kind,
                             Y[t].T.copy(), W[t].T.copy())
        kb, (_, _, nobs, ll) = loglik_bound(case)
        tol += kb + state_error_term(case, T * bx, T * bP)
        dof += nobs
        per_date += ll
    ev = {key: v.cpu().numpy() for key, v in kf.evidence.items()}
    assert np.array_equal(ev["dof"], dof) and np.all(ev["skipped"] == 0) and np.mean(dof > 0) > 0.9
    # the float64 batch formula cancels terms of order 1e2 to 1e3 (x0^T L0 x0, the log determinants) at 2^-53
    tol += 1e-10
    err = np.abs(ev["loglik"] - want)
    print(f"{form} {device}: loglik in [{want.min():.2f}, {want.max():.2f}], max err/tol {np.max(err / tol):.3f} "
          f"(tol up to {tol.max():.2e}, state error x {bx / U:.0f} u, P {bP / U:.0f} u); float64 per-date sum on the "
          f"engine's forecasts off the batch value by up to {np.max(np.abs(per_date - want)):.2e}")
    assert np.all(err <= tol)
    s = kf.evidence_summary()
    assert s["dof"] == int(dof.sum()) and s["skipped_pixel_dates"] == 0
    assert s["loglik"] == pytest.approx(float(ev["loglik"].sum()), rel=1e-12)
    assert s["d2_per_dof"] == pytest.approx(float(ev["d2"].sum()) / dof.sum(), rel=1e-12)
    return kf


@pytest.mark.parametrize("form", ["information", "gain"])
def test_engine_loglik_equals_batch_log_density(tmp_path, form):
    check_engine_prediction_error_decomposition(tmp_path, form)


@pytest.mark.parametrize("form,encoding,scope", [("information", "f32", "group"), ("gain", "bf16y", "band")])
def test_engine_gated_evidence_equals_run_on_edited_source(form, encoding, scope):
    """The construction of test_innovation's gated-run test: the evidence of a
    gated run is that of the observations it assimilated, bit for bit the
    accumulators of the ungated run on a source with the rejected observations
    set to nodata."""
    s = engine_setup(seed=4, encoding=encoding)
    mask, grid, obs = s[:3]
    rec = {}
    kf_a, _, _ = engine_run(*s, record=rec, analysis_form=form, innovation_gate=1.5, innovation_scope=scope,
                            innovation_evidence=True)
    assert sum(int(r.sum()) for d in rec.values() for r in d["reject"]) > 20

    def edit(date, bands):
        if date not in rec:
            return bands
        res = []
        for b, db in enumerate(bands):
            plane = getattr(db, PLANE[db.kind]).clone()
            code = NODATA[db.kind]
            plane[rec[date]["reject"][b]] = code - 65536 if code > 32767 else code
            res.append(dataclasses.replace(db, **{PLANE[db.kind]: plane}))
        return res
    kf_b, _, _ = engine_run(mask, grid, EditedSource(obs, edit), *s[3:], innovation_evidence=True, **unfused_cfg(form))
    assert set(kf_a.evidence) == {"loglik", "d2", "dof", "skipped"}
    for key in kf_a.evidence:
        assert torch.equal(kf_a.evidence[key], kf_b.evidence[key]), key
    kept = sum((d["stats"]["nobs"] - d["stats"]["nrej"]).to(torch.int32) for d in rec.values())
    assert torch.equal(kf_a.evidence["dof"], kept) and int(kf_a.evidence["skipped"].sum()) == 0
    assert kf_a.evidence_summary() == kf_b.evidence_summary()
    # the per-date nobs / nrej are still those of the first launch
    last = rec[max(rec)]["stats"]
    assert torch.equal(kf_a.last_innovation["nobs"], last["nobs"]) and int(last["nrej"].sum()) > 0


# ---------------------------------------------------------------- scan-q
TRUE_Q = 0.04          # cli run --sensor identity: TLAI's model error per step
SCALES = (1.0 / 16.0, 1.0, 16.0)


class WalkIdentity(k.SyntheticIdentityObservations):
    """Identity observations of a truth drawn from the filter's own model: on
    every date the six reset parameters from the JRC-TIP prior, TLAI a random
    walk from its prior with variance TRUE_Q per step; noise drawn at the
    declared uncertainty (float32 y / w pairs), a fifth of the pixel-dates
    without observations."""

    def __init__(self, state_mask, **kw):
        kw.update(encoding="f32", stream=False)
        kw.pop("cloud_fraction", None)
        super().__init__(state_mask, **kw)
        rng = np.random.default_rng(self.seed + 17)
        mu = k.JRCPrior(k.TIP_PARAMETERS, self.state_mask).mean      # the CLI's first forecast
        cov = k.tip_prior()[1]
        N, T = self.N, self.n_pool
        x = rng.multivariate_normal(mu, cov, size=(T, N))
        x[:, :, 6] = x[0, :, 6][None, :] + np.concatenate(
            [np.zeros((1, N)), np.cumsum(np.sqrt(TRUE_Q) * rng.standard_normal((T - 1, N)), axis=0)])
        self.sigma = np.where(np.arange(7) == 6, 0.05, 0.5 * np.sqrt(np.diag(cov)))
        y = x + self.sigma * rng.standard_normal(x.shape)
        seen = rng.random((T, N)) > 0.2
        w = np.where(seen[:, :, None], 1.0 / self.sigma ** 2, 0.0)
        self._yw = np.ascontiguousarray(np.concatenate([y.transpose(0, 2, 1), w.transpose(0, 2, 1)], axis=1),
                                        dtype=np.float32)

    def _synthesize(self, kk):
        return torch.from_numpy(self._yw[kk]).to(self.device)


def oracle_scan(src, dates, scale):
    """Float64 filter of the CLI's identity run (TIP prior as the first forecast;
    between dates every parameter reset to the prior except TLAI, carried with
    its precision inflated: P_f^-1[6, 6] = 1 / (1 / P_a^-1[6, 6] + q)) over the
    source's decoded observations: (total log evidence, d2, dof, summed kernel bound)."""
    mu, _, cinv = k.tip_prior()
    N, n = src.N, 7
    q = float(np.float32(TRUE_Q * scale))
    first = k.JRCPrior(k.TIP_PARAMETERS, src.state_mask).device_prior(None)     # the CLI's first forecast
    xf = np.tile(np.asarray(first.mean, dtype=np.float32).astype(np.float64), (N, 1))
    Pi = np.broadcast_to(np.asarray(first.cinv, dtype=np.float32).astype(np.float64), (N, n, n)).copy()
    tot = np.zeros(4)
    for d in dates:
        yw = [src.get_device_band_data(d, b).decode() for b in range(n)]
        y = np.stack([t[0].cpu().numpy()[:N].astype(np.float64) for t in yw])
        w = np.stack([t[1].cpu().numpy()[:N].astype(np.float64) for t in yw])
        case = identity_case(xf, Pi, "precision", y, w)
        kb, (d2, _, nobs, ll) = loglik_bound(case)
        tot += [ll.sum(), d2.sum(), nobs.sum(), kb.sum()]
        A = Pi + np.einsum("bp,bc->pbc", w, np.eye(n))
        xa = np.linalg.solve(A, (np.einsum("pij,pj->pi", Pi, xf) + (w * y).T)[:, :, None])[:, :, 0]
        xf = np.tile(mu, (N, 1))
        xf[:, 6] = xa[:, 6]
        Pi = np.broadcast_to(np.asarray(cinv, dtype=np.float32).astype(np.float64), (N, n, n)).copy()
        Pi[:, 6, 6] = 1.0 / (1.0 / A[:, 6, 6] + q)
    return tot


def test_cli_scan_q_picks_the_true_scale(monkeypatch, capsys):
    from kafka_inferenceengine_amd.cli import main
    steps, size = 6, (12, 10)
    src = WalkIdentity(np.ones(size, bool), device="cpu", seed=3)
    dates = sorted(src.dates)[:steps]
    want = {s: oracle_scan(src, dates, s) for s in SCALES}
    bound = sum(v[3] for v in want.values())
    margin = min(want[1.0][0] - want[s][0] for s in SCALES if s != 1.0)
    print(f"oracle: loglik {[round(want[s][0], 2) for s in SCALES]}, margin {margin:.2f}, summed bound {bound:.2e}")
    assert margin >= 10.0 * bound        # a condition on the inputs
    monkeypatch.setattr(k, "SyntheticIdentityObservations", WalkIdentity)
    main(["run", "--sensor", "identity", "--size", str(size[0]), str(size[1]), "--steps", str(steps), "--seed", "3",
          "--device", "cpu", "--scan-q"] + [repr(s) for s in SCALES])
    lines = [json.loads(ln) for ln in capsys.readouterr().out.strip().splitlines() if ln.startswith("{")]
    recs, choice = lines[:-1], lines[-1]
    assert [r["q_scale"] for r in recs] == list(SCALES) and choice["best_q_scale"] == 1.0
    for r in recs:
        ll, d2, dof, kb = want[r["q_scale"]]
        print(f"scale {r['q_scale']}: loglik {r['loglik']:.4f} (oracle {ll:.4f}, bound {kb:.2e}), "
              f"d2/dof {r['d2_per_dof']:.4f}")
        assert abs(r["loglik"] - ll) <= kb and r["dof"] == int(dof)
        assert abs(r["d2_per_dof"] - d2 / dof) <= 2.0 * kb / dof
    assert 0.8 < recs[1]["d2_per_dof"] < 1.2      # the consistency test at the true Q


def test_cli_scan_q_refusals(tmp_path):
    from kafka_inferenceengine_amd.cli import main
    base = ["run", "--sensor", "identity", "--size", "8", "8", "--steps", "2", "--device", "cpu", "--scan-q", "1", "2"]
    for extra in (["--out", str(tmp_path / "o")], ["--smooth-out", str(tmp_path / "s")],
                  ["--resume", str(tmp_path / "r")]):
        with pytest.raises(SystemExit, match="scan-q"):
            main(base + extra)
    with pytest.raises(SystemExit, match="q-scale"):
        main(["run", "--sensor", "identity", "--size", "8", "8", "--steps", "2", "--device", "cpu", "--q-scale", "0"])
    with pytest.raises(SystemExit, match="without a model error"):
        main(["run", "--sensor", "s1", "--size", "8", "8", "--steps", "2", "--device", "cpu", "--q-scale", "2"])


# ------------------------------------------------- outputs, refusals, defaults
def test_evidence_rasters_read_back_equal_to_the_accumulators(tmp_path):
    from kafka_inferenceengine_amd.input_output.evidence import write_evidence_rasters
    s = engine_setup(seed=4)
    mask = s[0]
    kf, _, _ = engine_run(*s, innovation_gate=1.5, innovation_evidence=True)
    gt = [500000.0, 30.0, 0.0, 4100000.0, 0.0, -30.0]
    paths = write_evidence_rasters(str(tmp_path / "ev"), kf, gt, "")
    assert [os.path.basename(p) for p in paths] == ["evidence_loglik.tif", "evidence_d2_per_dof.tif",
                                                    "evidence_dof.tif", "evidence_rejected_dates.tif"]
    ev = {key: v.cpu().numpy() for key, v in kf.evidence.items()}
    with np.errstate(all="ignore"):
        want = [ev["loglik"], np.where(ev["dof"] > 0, ev["d2"] / ev["dof"], np.nan), ev["dof"],
                kf.gate_history.cpu().numpy()]
    for p, w in zip(paths, want):
        r, info = k.read_tiff(p)
        assert r.dtype == np.float32 and r.shape == mask.shape and list(info["geotransform"]) == gt
        assert np.isnan(r[~mask]).all()
        assert np.array_equal(r[mask], w.astype(np.float32), equal_nan=True), p
    assert int(kf.gate_history.sum()) > 0 and np.isfinite(ev["loglik"]).all()
    # a pixel that never had an observation: dof 0, d2 per dof NaN, log evidence 0
    kf.evidence["dof"][0] = 0
    paths = write_evidence_rasters(str(tmp_path / "ev0"), kf, gt, "")
    assert np.isnan(k.read_tiff(paths[1])[0][mask][0]) and k.read_tiff(paths[2])[0][mask][0] == 0.0


def test_cli_run_evidence_out(tmp_path, capsys):
    from kafka_inferenceengine_amd.cli import main
    base = ["run", "--sensor", "bhr", "--size", "24", "20", "--steps", "3", "--n-train", "40", "--device", "cpu"]
    main(base + ["--evidence-out", str(tmp_path / "a"), "--q-scale", "2"])
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert sorted(os.listdir(tmp_path / "a")) == ["evidence_d2_per_dof.tif", "evidence_dof.tif", "evidence_loglik.tif"]
    ev = rec["evidence"]
    assert set(ev) == {"loglik", "d2", "dof", "d2_per_dof", "skipped_pixel_dates", "files"} and ev["dof"] > 0
    ll = k.read_tiff(tmp_path / "a" / "evidence_loglik.tif")[0]
    assert ll.shape == (24, 20) and float(ll.astype(np.float64).sum()) == pytest.approx(ev["loglik"], rel=1e-5)
    assert k.read_tiff(tmp_path / "a" / "evidence_dof.tif")[0].sum() == ev["dof"]
    main(base + ["--evidence-out", str(tmp_path / "b"), "--innovation-gate", "2.5"])
    rec_b = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert sorted(os.listdir(tmp_path / "b")) == ["evidence_d2_per_dof.tif", "evidence_dof.tif", "evidence_loglik.tif",
                                                  "evidence_rejected_dates.tif"]
    assert rec_b["evidence"]["dof"] <= k.read_tiff(tmp_path / "b" / "evidence_dof.tif")[0].sum() + 0.5
    main(base)                                  # no option: no evidence in the record
    assert "evidence" not in json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_engine_evidence_refusals():
    mask, grid, obs, x0, Pinv, Q = engine_setup(seed=5)
    opt = dict(innovation_evidence=True)
    with pytest.raises(ValueError, match="band_sequential"):
        _engine(mask, obs, Q, band_sequential=True, **opt).run(grid, x0, None, Pinv)
    with pytest.raises(ValueError, match="band_parallel"):
        _engine(mask, obs, Q, band_parallel=2, band_parallel_force=True, **opt).run(grid, x0, None, Pinv)

    def user_factory(*a):      # no device_spec: evaluated on the host, OP_PRECOMP bands
        return k.create_nonlinear_observation_operator(*a)
    obs.band_spec = lambda date, band: None
    kf = k.LinearKalman(obs, None, mask, user_factory, k.TIP_PARAMETERS, device="cpu",
                        state_propagation=k.propagate_information_filter_LAI, config=k.EngineConfig(**opt))
    kf.set_trajectory_model()
    kf.set_trajectory_uncertainty(Q)
    with pytest.raises(ValueError, match="operator"):
        kf.run(grid, x0, None, Pinv)
    with pytest.raises(ValueError, match="operator"):
        kf.innovation(kf.initial_state(x0, None, Pinv), grid[0], joint=True)


@pytest.mark.parametrize("form", ["information", "gain"])
def test_defaults_unchanged_and_evidence_changes_no_output(form):
    """Every new option off: the keys of last_innovation and the run's outputs
    are what they were; the option on changes no output of the run, and
    LinearKalman.innovation returns d2 / logdet only when asked."""
    s = engine_setup(seed=3)
    rec = {}
    a = engine_run(*s, analysis_form=form, innovation_stats=True)
    b = engine_run(*s, record=rec, analysis_form=form, innovation_evidence=True)
    c = engine_run(*s, **unfused_cfg(form))
    same_run(a, b)
    same_run(a, c)
    assert a[0].evidence is None and c[0].evidence is None and c[0].last_innovation is None
    assert set(a[0].last_innovation) == {"chi2", "nobs", "nrej", "status"}
    assert set(b[0].last_innovation) == {"chi2", "nobs", "nrej", "status", "d2", "logdet"}
    for key in ("chi2", "nobs", "nrej", "status"):
        assert torch.equal(a[0].last_innovation[key], b[0].last_innovation[key])
    assert a[0].evidence_summary() == {"loglik": 0.0, "d2": 0.0, "dof": 0, "d2_per_dof": None, "skipped_pixel_dates": 0}
    kf = b[0]
    from kafka_inferenceengine_amd.engine.state import KFState
    date = max(rec)
    d = rec[date]
    fc = KFState(d["x"].clone(), d["P"].clone(), d["kind"], kf.N)
    plain = kf.innovation(fc, date)
    joint = kf.innovation(fc, date, joint=True)
    assert set(plain) == {"z", "chi2", "nobs", "nrej", "status"} and set(joint) == set(plain) | {"d2", "logdet"}
    for key in plain:
        assert torch.equal(plain[key], joint[key]) or key == "z" and torch.equal(torch.nan_to_num(plain[key]),
                                                                                   torch.nan_to_num(joint[key]))
    assert torch.equal(joint["d2"], d["stats"]["d2"]) and torch.equal(joint["logdet"], d["stats"]["logdet"])
    # the run's accumulators are the per-date values summed in float64
    ev = kf.evidence
    assert int(ev["skipped"].sum()) == 0
    assert int(ev["dof"].sum()) == sum(int(r["stats"]["nobs"].sum()) for r in rec.values())
    ll = sum(-0.5 * (r["stats"]["d2"].double() + r["stats"]["logdet"].double() + r["stats"]["nobs"].double() * LOG2PI)
             for r in rec.values())
    assert torch.allclose(ev["loglik"], ll, rtol=1e-12, atol=1e-12)


def test_metrics_record_carries_the_joint_statistic(tmp_path):
    s = engine_setup(seed=4)
    rec = {}
    path = tmp_path / "metrics.jsonl"
    kf, _, _ = engine_run(*s, record=rec, innovation_evidence=True, metrics_path=str(path))
    per_date = [json.loads(ln)["innovation"] for ln in open(path) if json.loads(ln).get("event") == "date"]
    assert len(per_date) == 4
    for date, m in zip(sorted(rec), per_date):
        st = rec[date]["stats"]
        nobs = int(st["nobs"].sum())
        d2, ld = float(st["d2"].double().sum()), float(st["logdet"].double().sum())
        assert set(m) == {"observed", "rejected", "unscreenable", "chi2_per_obs", "d2_per_obs", "loglik"}
        assert m["d2_per_obs"] == pytest.approx(d2 / nobs, rel=1e-9)
        assert m["loglik"] == pytest.approx(-0.5 * (d2 + ld + nobs * LOG2PI), rel=1e-9)
    assert sum(m["loglik"] for m in per_date) == pytest.approx(kf.evidence_summary()["loglik"], rel=1e-9)


# ------------------------------------------------------------------ 2 ranks
def _rank_evidence(world, rank, q):
    from kafka_inferenceengine_amd.parallel import Comm, StripPartition

    if world > 1:
        torch.set_num_threads(1)
    mask = mask_with_holes((30, 22))
    comm = Comm(rank, world, "cpu") if world > 1 else Comm.single("cpu")
    part = StripPartition(mask, rank, world)
    obs = k.SyntheticBHRObservations(mask, n_train=60, stream=False, n_pool=4, device="cpu", seed=4, field_cell=8,
                                     encoding="f32", partition=part)
    kf = k.LinearKalman(obs, None, mask, k.create_nonlinear_observation_operator, k.TIP_PARAMETERS,
                        state_propagation=k.propagate_information_filter_LAI, device="cpu", comm=comm, partition=part,
                        config=k.EngineConfig(innovation_evidence=True, innovation_gate=2.0))
    kf.set_trajectory_model()
    kf.set_trajectory_uncertainty(np.array([0, 0, 0, 0, 0, 0, 0.04]))
    kf.run(_grid(4), kf.state_from_prior(k.JRCPrior(k.TIP_PARAMETERS, mask)), None, None)
    q.put((rank, kf.evidence_summary(), {key: v.numpy() for key, v in kf.evidence.items()}))


def _rank_evidence_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _rank_evidence(world, rank, q)
    finally:
        dist.destroy_process_group()


def test_evidence_summary_two_ranks_equal_one_rank():
    """The per-pixel accumulators of two strips are those of the one-rank run bit
    for bit; the summary's counts are equal, its float64 totals equal up to the
    order of the additions (two partial sums against one)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    _rank_evidence(1, 0, q)
    _, one, ev1 = q.get()
    port = _free_port()
    procs = [ctx.Process(target=_rank_evidence_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=300) for _ in range(2)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0][1] == res[1][1]
    two = res[0][1]
    for key in ev1:
        assert np.array_equal(np.concatenate([r[2][key] for r in res]), ev1[key]), key
    assert two["dof"] == one["dof"] > 0 and two["skipped_pixel_dates"] == one["skipped_pixel_dates"]
    for key in ("loglik", "d2", "d2_per_dof"):
        assert two[key] == pytest.approx(one[key], rel=1e-12)
