"""Physical-unit product rasters with credible intervals and the QA byte: the
per-pixel pass on the host runner against float64
(``inference.kf_tools.product_blocks``), the failure rule, the exact-boundary
cases, and the outputs / engine / smoother / CLI with ``physical=`` and
``qa=``.

Truth is numpy float64 on the float32-rounded inputs and the float32 z.  With
U = 2^-24, u_c the oracle's clamped argument, sigma the marginal std and
eps_sigma the bound on its relative error (``test_marginal.marginal_truth``
for precision rows, 2 U for covariance rows), per value

    neglog:            |d phys| <= 2 |scale| (z sigma eps_sigma / u_c + U (1 + 3 |ln u_c|))
    linear / identity: |d phys| <= 2 (|scale| (z sigma eps_sigma + U |u_c|) + U |phys|)

(the argument's error through the transform's slope, one rounding of the
argument, a logarithm good to under 3 ulp, one rounding of the result; for the
median sigma = 0).  The QA bytes must be the oracle's exactly, so the inputs
are drawn unambiguous: x of a pixel is redrawn while a float64 x_j, u- or u+
lies within 64 (z sigma eps_sigma + U |u|) of a bound."""
import datetime as dt
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.inference.kf_tools import product_blocks
from kafka_inferenceengine_amd.ops import kernels as K

from test_engine import _engine, _grid, _setup
from test_marginal import SIZES, U, blocks_of, marginal_truth, pack_rows, problem, spd_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7.0
Z95 = k.credible_z(0.95)
T = k.ParameterTransform


def mixed_table(n):
    """All three kinds in turn over the selected parameters, one parameter left
    out (none at n = 1): the last but one, so a selected one follows the gap."""
    kinds = (T("neglog", scale=2.0, lo=np.exp(-5.0), hi=1.0), T("linear", scale=90.0, offset=-3.0, lo=0.0, hi=1.0),
             T("identity"), T("neglog", scale=0.02, lo=0.05, hi=0.9), T("linear", scale=-2.5, offset=1.0))
    out, s = [], 0
    for j in range(n):
        if n > 1 and j == max(n - 2, 1):
            out.append(None)
            continue
        out.append(kinds[s % len(kinds)])
        s += 1
    return out


def sigma_truth(A, kind):
    """Marginal std [N, n] in float64 and the bound on its relative error [N]."""
    if kind == "covariance":
        return np.sqrt(np.diagonal(A, axis1=1, axis2=2)), np.full(A.shape[0], 2 * U)
    return marginal_truth(A)


def product_problem(n, N, seed, kind, table, z, device="cpu", bad=None):
    """The raster map, plane and row stride of ``test_marginal.problem``; blocks
    from ``spd_blocks`` rescaled per parameter so that the marginal std is
    log-uniform in [0.005, 0.5]; a third of the pixels quiet (x well inside
    [0.3, 0.7], a small sigma: nothing clamped), the others with x in
    [-0.3, 1.3].  ``bad``: a pixel whose block is made -I (precision) or whose
    last selected variance is negated (covariance).  x is redrawn until no
    pixel is ambiguous against a bound."""
    _, _, idx, plane = problem(n, 1e3, N, seed, device)
    ld = N + 3
    rng = np.random.default_rng(seed + 17)
    A = spd_blocks(n, 1e3, N, seed)
    sd0 = np.sqrt(np.diagonal(np.linalg.inv(A) if kind == "precision" else A, axis1=1, axis2=2))
    quiet = rng.random(N) < 1.0 / 3.0
    target = np.exp(rng.uniform(np.log(0.005), np.log(0.5), (N, n)))
    target[quiet] = np.exp(rng.uniform(np.log(0.005), np.log(0.02), (int(quiet.sum()), n)))
    s = target / sd0
    A = A / (s[:, :, None] * s[:, None, :]) if kind == "precision" else A * s[:, :, None] * s[:, None, :]
    p = pack_rows(A, ld)
    A32 = blocks_of(p, n, N)
    sd, eps = sigma_truth(A32, kind)
    sel = [j for j, t in enumerate(table) if t is not None]
    if bad is not None:
        iu = np.triu_indices(n)
        diag_rows = np.nonzero(iu[0] == iu[1])[0]
        if kind == "precision":
            p[:, bad] = 0.0
            p[diag_rows, bad] = -1.0
        else:
            p[diag_rows[sel[-1]], bad] *= -1.0

    def draw(m, q):
        return np.where(q[:, None], rng.uniform(0.3, 0.7, (m, n)), rng.uniform(-0.3, 1.3, (m, n))).astype(np.float32)

    x = draw(N, quiet)
    for _ in range(64):
        amb = np.zeros(N, bool)
        for j in sel:
            _, _, lo, hi = table[j].f32()
            xj = x[:, j].astype(np.float64)
            for u in (xj, xj - z * sd[:, j], xj + z * sd[:, j]):
                margin = 64.0 * (z * sd[:, j] * eps + U * np.abs(u))
                for b in (lo, hi):
                    if np.isfinite(b):
                        amb |= np.abs(u - b) <= margin
        if not amb.any():
            break
        x[amb] = draw(int(amb.sum()), quiet[amb])
    else:
        raise AssertionError("could not draw unambiguous inputs")
    xs = np.zeros((n, ld), np.float32)
    xs[:, :N] = x.T
    return (torch.from_numpy(xs).to(device), torch.from_numpy(p).to(device), idx, plane, sd, eps)


def run_product(n, x, p, table, z, idx, plane, N, kind, status=None, nobs=None, nrej=None, qa=True):
    n_sel = sum(t is not None for t in table)
    phys = torch.full((3 * n_sel, plane), SENTINEL, dtype=torch.float32, device=x.device) if n_sel else None
    q = torch.full((plane,), 255, dtype=torch.uint8, device=x.device) if qa else None
    K.product(n, x, p, table, z, phys=phys, qa=q, idx=idx, N=N, kind=kind, status=status, nobs=nobs, nrej=nrej)
    return (None if phys is None else phys.cpu().numpy()), (None if q is None else q.cpu().numpy())


def value_bound(t, u_c, phys, zs_eps):
    """The docstring's bound per value; zs_eps = z sigma eps_sigma (0 for the median)."""
    scale = abs(t.f32()[0])
    if t.kind == "neglog":
        return 2.0 * scale * (zs_eps / u_c + U * (1.0 + 3.0 * np.abs(np.log(u_c))))
    return 2.0 * (scale * (zs_eps + U * np.abs(u_c)) + U * np.abs(phys))


def check_product(n, N, seed, kind, device="cpu", z=Z95, seen=None):
    """One problem against float64: values within the bound, NaN where the
    oracle has NaN, QA bytes equal on every pixel, sentinels untouched."""
    table = mixed_table(n)
    sel = [j for j, t in enumerate(table) if t is not None]
    n_sel = len(sel)
    bad = N // 2 if N >= 3 else None
    x, p, idx, plane, sd, eps = product_problem(n, N, seed, kind, table, z, device, bad=bad)
    rng = np.random.default_rng(seed + 5)
    st_bits = np.array([0, 0, K.ST_NO_OBS, K.ST_FALLBACK, K.ST_NONSPD, K.ST_OUT_OF_DOMAIN, K.ST_NO_OBS | K.ST_BAD_OP,
                        K.ST_NONFINITE | K.ST_OUT_OF_DOMAIN], np.uint8)
    status = st_bits[rng.integers(0, st_bits.size, N)]
    nobs = rng.integers(0, 3, N).astype(np.uint8)
    nrej = np.minimum(nobs, rng.integers(0, 3, N)).astype(np.uint8)
    dev_in = [torch.from_numpy(a).to(device) for a in (status, nobs, nrej)]
    phys, qa = run_product(n, x, p, table, z, idx, plane, N, kind, *dev_in)
    A = blocks_of(p.cpu().numpy(), n, N)
    med, lower, upper, qa_ref, clamped = product_blocks(x.cpu().numpy()[:, :N].T, A, table, z, kind=kind,
                                                        status=status, nobs=nobs, nrej=nrej)
    ii = idx.cpu().numpy()
    rest = np.setdiff1d(np.arange(plane), ii)
    assert np.array_equal(qa[ii], qa_ref), f"QA differs on {np.count_nonzero(qa[ii] != qa_ref)} of {N} pixels"
    assert np.all(qa[rest] == 255) and np.all(phys[:, rest] == SENTINEL)
    worst = 0.0
    for s, j in enumerate(sel):
        t = table[j]
        zs_eps = z * sd[:, j] * eps
        for g, (ref, zz) in enumerate(((med, 0.0), (lower, 1.0), (upper, 1.0))):
            got = phys[g * n_sel + s, ii].astype(np.float64)
            want = ref[:, s]
            assert np.array_equal(np.isnan(got), np.isnan(want))
            fin = ~np.isnan(want)
            if g == 0:
                u_c = clamped[0, :, s]
            else:
                # lower / upper: the end whose transform the oracle picked
                f1 = t.apply(clamped[1, :, s])
                pick_m = (f1 == want)
                u_c = np.where(pick_m, clamped[1, :, s], clamped[2, :, s])
            bound = value_bound(t, u_c[fin], want[fin], zz * zs_eps[fin])
            err = np.abs(got[fin] - want[fin])
            if err.size:
                worst = max(worst, float(np.max(err / bound)))
            assert np.all(err <= bound), (kind, j, g, float(np.max(err / bound)))
    print(f"n={n} N={N} {kind}: max err/bound {worst:.3f}")
    if seen is not None:
        for bit in (4, 5, 6):
            hit = (qa_ref >> bit) & 1
            seen[bit][0] |= bool(hit.any())
            seen[bit][1] |= bool((hit == 0).any())
    return phys, qa


def new_seen():
    return {bit: [False, False] for bit in (4, 5, 6)}


def assert_seen(seen):
    """The inputs set each of the bits 4, 5, 6 somewhere and leave each clear somewhere."""
    for bit, (on, off) in seen.items():
        assert on and off, f"QA bit {bit}: set somewhere {on}, clear somewhere {off}"


def check_failure_rule(n, N, seed, device="cpu"):
    """The -I and NaN-entry blocks of ``test_marginal.check_failure_rule``: NaN in
    that pixel's ends only, its medians intact, bit 4 there and nowhere else."""
    table = [T("identity")] * n
    iu = np.triu_indices(n)
    diag_rows = np.nonzero(iu[0] == iu[1])[0]
    for case in ("minus_identity", "nan_entry"):
        x, p, idx, plane = problem(n, 1e3, N, seed, device)
        bad = N // 2
        if case == "minus_identity":
            p[:, bad] = 0.0
            p[diag_rows, bad] = -1.0
        else:
            p[p.shape[0] - 1 if n == 1 else 1, bad] = float("nan")
        phys, qa = run_product(n, x, p, table, Z95, idx, plane, N, "precision")
        ii = idx.cpu().numpy()
        assert np.array_equal(phys[:n, ii], x.cpu().numpy()[:, :N]), case       # the medians: x, bit for bit
        nan = np.isnan(phys[n:, ii])
        assert nan[:, bad].all() and nan.sum() == 2 * n, case
        want = np.zeros(N, np.uint8)
        want[bad] = 16
        assert np.array_equal(qa[ii], want), case


def check_boundaries(device="cpu"):
    """x == hi: phys == 0 exactly and bit 5 clear; one ulp above: the same phys, bit 5 set."""
    n, N = 2, 4
    table = [T("neglog", scale=2.0, lo=np.exp(-5.0), hi=1.0), None]
    x = np.full((n, N), 0.5, np.float32)
    x[0, 1] = 1.0
    x[0, 2] = np.nextafter(np.float32(1.0), np.float32(2.0))
    x[0, 3] = np.float32(np.exp(-5.0))                       # == lo
    p = pack_rows(np.broadcast_to(np.eye(n) * 1e4, (N, n, n)).copy(), N)       # sigma = 0.01
    phys, qa = run_product(n, torch.from_numpy(x).to(device), torch.from_numpy(p).to(device), table, Z95, None, N, N,
                           "precision")
    assert phys[0, 1] == 0.0 and phys[0, 2] == 0.0 and not (qa[1] & 32) and (qa[2] & 32)
    assert phys[1, 1] == 0.0 and (qa[1] & 64) and (qa[2] & 64)          # the lower end: the clamped upper argument
    assert not (qa[3] & 32) and (qa[3] & 64) and qa[0] == 0
    assert abs(phys[0, 3] - 10.0) <= 10.0 * 8 * U and phys[2, 3] == phys[0, 3]


# ---------------------------------------------------------------- kernel (host runner)
@pytest.mark.parametrize("kind", ["precision", "covariance"])
@pytest.mark.parametrize("n", SIZES)
def test_product_host_runner_against_float64(n, kind):
    seen = new_seen()
    check_product(n, 257, seed=31 * n, kind=kind, seen=seen)
    assert_seen(seen)


@pytest.mark.parametrize("n", SIZES)
def test_product_failure_rule(n):
    check_failure_rule(n, 257, seed=n)


def test_product_exact_boundaries():
    check_boundaries()


def test_product_qa_only_and_null_inputs():
    """No transform: the QA plane alone; null status / nobs / nrej leave their bits clear."""
    n, N = 3, 40
    x, p, idx, plane = problem(n, 1e3, N, 3)
    p[:, 7] = 0.0
    _, qa = run_product(n, x, p, [None] * n, Z95, idx, plane, N, "precision")
    want = np.zeros(N, np.uint8)
    want[7] = 16
    assert np.array_equal(qa[idx.numpy()], want)
    status = torch.full((N,), K.ST_NO_OBS, dtype=torch.uint8)
    _, qa = run_product(n, x, p, [None] * n, Z95, idx, plane, N, "covariance", status=status)
    assert np.all(qa[idx.numpy()] == 1)
    phys, none = run_product(n, x, p, [T("identity")] * n, Z95, idx, plane, N, "covariance", qa=False)
    assert none is None and np.array_equal(phys[:n, idx.numpy()], x.numpy()[:, :N])


def test_product_argument_checks():
    x, p, idx, plane = problem(3, 10.0, 20, 0)
    table = [T("identity"), None, T("linear", scale=2.0)]
    phys = torch.zeros((6, plane))
    qa = torch.zeros(plane, dtype=torch.uint8)
    K.product(3, x, p, table, Z95, phys=phys, qa=qa, idx=idx, N=20)
    with pytest.raises(ValueError):
        K.product(3, x, p, table, Z95, phys=phys, qa=qa, idx=idx, N=20, kind="variance")
    with pytest.raises(ValueError):
        K.product(5, x, p, table, Z95, phys=phys, qa=qa, idx=idx, N=20)
    with pytest.raises(ValueError):
        K.product(3, x, p[:5], table, Z95, phys=phys, qa=qa, idx=idx, N=20)
    with pytest.raises(ValueError):
        K.product(3, x, p, table[:2], Z95, phys=phys, qa=qa, idx=idx, N=20)
    with pytest.raises(ValueError):
        K.product(3, x, p, table, Z95, phys=torch.zeros((9, plane)), qa=qa, idx=idx, N=20)     # 3 n_sel planes
    with pytest.raises(ValueError):
        K.product(3, x, p, table, Z95, phys=phys, qa=torch.zeros(plane + 1, dtype=torch.uint8), idx=idx, N=20)
    with pytest.raises(ValueError):
        K.product(3, x, p, table, Z95, phys=torch.zeros((6, 10)), N=20)      # plane < N without an index map
    with pytest.raises(ValueError):
        K.product(3, x, p, table, 0.0, phys=phys, qa=qa, idx=idx, N=20)
    with pytest.raises(ValueError):
        K.product(3, x, p, table, Z95, phys=phys, qa=qa, idx=idx, N=20, status=torch.zeros(20, dtype=torch.int32))
    with pytest.raises(ValueError):
        K.product(3, x, p, table, Z95, idx=idx, N=20)
    with pytest.raises(TypeError):
        K.product(3, x, p.double(), table, Z95, phys=phys, qa=qa, idx=idx, N=20)


def test_transform_checks_and_level():
    with pytest.raises(ValueError):
        T("neglog", scale=2.0, lo=0.0, hi=1.0)
    with pytest.raises(ValueError):
        T("neglog", scale=2.0, lo=-1.0, hi=1.0)
    with pytest.raises(ValueError):
        T("neglog", scale=2.0, lo=0.1)                       # hi = inf
    with pytest.raises(ValueError):
        T("log")
    with pytest.raises(ValueError):
        T("linear", lo=2.0, hi=1.0)
    for level in (0.0, 1.0, -0.5, 1.5):
        with pytest.raises(ValueError):
            k.credible_z(level)
    assert k.credible_z(0.95) == float(np.float32(1.959963984540054))
    assert k.TIP_TRANSFORMS["TeLAI"].physical_range() == pytest.approx((0.0, 10.0), abs=1e-5)
    assert set(k.SAIL_TRANSFORMS) == {"cab", "car", "cw", "cm", "lai", "ala"}
    assert k.SAIL_TRANSFORMS["ala"].kind == "linear" and k.SAIL_TRANSFORMS["cw"].f32()[0] == float(np.float32(0.02))
    # names: a product may not take a parameter's name (any case) or another product's
    with pytest.raises(ValueError, match="collides"):
        k.DeviceOutput(k.TIP_PARAMETERS, physical={"TeLAI": T("identity", name="telai")})
    with pytest.raises(ValueError, match="twice"):
        k.KafkaOutputMemory(["a", "b"], physical={"a": T("identity", name="P"), "b": T("identity", name="p")})
    with pytest.raises(ValueError, match="level"):
        k.DeviceOutput(k.TIP_PARAMETERS, physical=k.TIP_TRANSFORMS, level=1.0)


# ---------------------------------------------------------------- engine / outputs
class Recording(k.DeviceOutput):
    """A DeviceOutput that keeps what every dump was handed: the state and the
    timestep's accumulated QA inputs (clones: the engine folds further dates into them)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.seen = {}

    def dump_state(self, timestep, state, engine, qa_inputs=None):
        self.seen[timestep] = (state, None if qa_inputs is None
                               else tuple(None if t is None else t.clone() for t in qa_inputs))
        super().dump_state(timestep, state, engine, qa_inputs=qa_inputs)


def product_of_state(kf, state, qa_inputs, table, z, n_sel):
    """K.product applied afterwards to a state, onto fresh planes of the strip."""
    dev = state.x.device
    H, W = kf.partition.strip_shape
    idx = torch.from_numpy(np.asarray(kf.partition.local_idx, dtype=np.int64)).to(dev)
    phys = torch.zeros((3 * n_sel, H * W), dtype=torch.float32, device=dev)
    qa = torch.full((H * W,), 255, dtype=torch.uint8, device=dev)
    st = kf._materialize(state)
    status, nobs, nrej = qa_inputs if qa_inputs is not None else (None, None, None)
    K.product(kf.n_params, st.x, st.P, table, z, phys=phys, qa=qa, idx=idx, N=state.N, kind=st.kind, status=status,
              nobs=nobs, nrej=nrej)
    return phys, qa


def engine_product_check(form, make_engine):
    """``make_engine(out, **cfg) -> (kf, run)``.  A run with products, QA and
    marginal rasters, gate on: the product planes of every date equal
    ``K.product`` applied afterwards to the state that date returned, with its
    accumulated status, bit for bit; the standard planes equal those of the
    same run without products.  Then one timestep without a date."""
    cfg = dict(analysis_form=form, innovation_gate=1.0)
    out = Recording(k.TIP_PARAMETERS, keep_history=True, uncertainty="marginal", physical=k.TIP_TRANSFORMS, qa=True)
    kf, run = make_engine(out, **cfg)
    st = run(kf)
    ref = k.DeviceOutput(k.TIP_PARAMETERS, keep_history=True, uncertainty="marginal")
    kf2, run2 = make_engine(ref, **cfg)
    st2 = run2(kf2)
    assert torch.equal(st.x, st2.x) and torch.equal(st.P, st2.P)
    assert sorted(out.history) == sorted(ref.history) == sorted(out.product_history) and len(out.history) >= 3
    table = out.products.table(7)
    mask = kf.partition.local_mask.reshape(-1)
    bits = 0
    for t in sorted(out.history):
        assert torch.equal(out.history[t][0], ref.history[t][0]) and torch.equal(out.history[t][1], ref.history[t][1])
        state, qa_in = out.seen[t]
        assert qa_in is not None and qa_in[0] is not None and qa_in[1] is not None and qa_in[2] is not None
        phys, qa = product_of_state(kf, state, qa_in, table, out.products.z, 1)
        got_p, got_q = out.product_history[t]
        assert torch.equal(got_p.view(torch.int32), phys.view(torch.int32)) and torch.equal(got_q, qa)
        q = got_q.cpu().numpy()
        assert np.all(q[~mask] == 255) and np.all(q[mask] < 128)
        assert np.array_equal((q[mask] & 8) != 0, qa_in[2][:state.N].cpu().numpy() > 0)
        p = got_p.cpu().numpy()
        fin = (q[mask] & 16) == 0
        assert np.all(p[:, ~mask] == 0) and fin.any()
        assert np.all((p[1, mask][fin] <= p[0, mask][fin]) & (p[0, mask][fin] <= p[2, mask][fin]))
        assert np.all((p[:, mask][:, fin] >= 0) & (p[:, mask][:, fin] <= 10.0 * (1 + 8 * U)))
        bits |= int(np.bitwise_or.reduce(q[mask]))
    print(f"{form}: QA bits seen over the run {bits:#04x}")
    # a timestep without a date: ST_NO_OBS everywhere and no other status bit
    t_next = max(out.history) + dt.timedelta(days=16)
    kf.step(t_next, [], st)
    state, qa_in = out.seen[t_next]
    assert qa_in[1] is None and qa_in[2] is None and torch.all(qa_in[0] == K.ST_NO_OBS)
    q = out.product_history[t_next][1].cpu().numpy()
    assert np.all((q[mask] & 0x0F) == 1) and np.all(q[~mask] == 255)
    # bits 4-6 speak of the products (after a propagation with Q the 95 % interval of TeLAI passes
    # hi = 1 on many pixels, which is bit 6): the QA layer on its own is 1 on every active pixel
    only = k.DeviceOutput(k.TIP_PARAMETERS, keep_history=True, qa=True)
    kf.output = only
    kf.step(t_next, [], st)
    assert only.product_history[t_next][0] is None
    q1 = only.product_history[t_next][1].cpu().numpy()
    assert np.all(q1[mask] == 1) and np.all(q1[~mask] == 255)
    return out, kf, st


def _cpu_engine(seed):
    mask, obs, prior, x0, Pinv, Q = _setup(seed=seed)
    grid = _grid(4)

    def make(out, **cfg):
        return _engine(mask, obs, Q, out=out, **cfg), lambda kf: kf.run(grid, x0, None, Pinv)
    return make, mask, grid


@pytest.mark.parametrize("form", ["information", "gain"])
def test_engine_product_output_equals_pass_on_returned_state(form):
    make, _, _ = _cpu_engine(seed=6)
    engine_product_check(form, make)


def test_product_with_spatial_prior_raises():
    mask, obs, prior, x0, Pinv, Q = _setup(seed=9)
    for kw in (dict(physical=k.TIP_TRANSFORMS), dict(qa=True)):
        out = k.DeviceOutput(k.TIP_PARAMETERS, **kw)
        kf = _engine(mask, obs, Q, out=out, spatial_gamma=50.0, spatial_params=[6], jacobi_sweeps=4)
        with pytest.raises(ValueError, match="spatial"):
            kf.run(_grid(3), x0, None, Pinv)


def check_standard_planes_equal_unfused_run(form, make_engine):
    """What the option does to the standard rasters: nothing beyond taking the
    unfused launches.  Default uncertainty, with products and QA, against
    ``fuse_output=False`` without them: state, mean and unc planes bit for bit,
    in both forms.  (Against the fused default the gain form differs in the last
    bits from the second date on: its fused launches store the precision
    diagonal for the next forecast, the unfused ones the covariance.)"""
    res = []
    for kw, cfg in ((dict(physical=k.TIP_TRANSFORMS, qa=True), {}), ({}, dict(fuse_output=False))):
        out = k.DeviceOutput(k.TIP_PARAMETERS, keep_history=True, **kw)
        kf, run = make_engine(out, analysis_form=form, **cfg)
        res.append((run(kf), out))
    (sa, oa), (sb, ob) = res
    assert torch.equal(sa.x, sb.x) and torch.equal(sa.P, sb.P)
    assert sorted(oa.history) == sorted(ob.history) and len(oa.history) >= 3
    for t in oa.history:
        assert torch.equal(oa.history[t][0], ob.history[t][0]) and torch.equal(oa.history[t][1], ob.history[t][1])


@pytest.mark.parametrize("form", ["information", "gain"])
def test_standard_planes_equal_unfused_run(form):
    make, _, _ = _cpu_engine(seed=6)
    check_standard_planes_equal_unfused_run(form, make)


def fold_qa(per):
    """Independent fold of per-analysis (status, nobs, nrej) numpy triples: ST_NO_OBS
    where every one has it, the other status bits where any has, saturating sums."""
    st = np.stack([a[0] for a in per]).astype(np.uint8)
    no_obs = np.bitwise_and.reduce(st & K.ST_NO_OBS, axis=0)
    other = np.bitwise_or.reduce(st & (0xFF ^ K.ST_NO_OBS), axis=0)
    if per[0][1] is None:
        return (no_obs | other).astype(np.uint8), None, None
    nobs = np.minimum(np.sum([a[1].astype(np.int64) for a in per], axis=0), 255).astype(np.uint8)
    nrej = np.minimum(np.sum([a[2].astype(np.int64) for a in per], axis=0), 255).astype(np.uint8)
    return (no_obs | other).astype(np.uint8), nobs, nrej


def check_qa_fold(make_engine, grid, per_step, **cfg):
    """Several analyses per timestep (dates, or the bands of a date under
    band_sequential): the QA inputs ``dump_state`` is handed equal an independent
    fold of what each analysis left in ``last_status`` / ``last_innovation``, and
    the QA plane equals the oracle's bits 0 to 3 of that fold."""
    out = Recording(k.TIP_PARAMETERS, keep_history=True, qa=True)
    kf, run = make_engine(out, **cfg)
    log = []
    inner = kf._qa_accumulate

    def spy():
        N = kf.N
        li = kf.last_innovation if kf._screening() else None
        log.append((kf.current_timestep, kf.last_status[:N].cpu().numpy().copy(),
                    None if li is None else li["nobs"].cpu().numpy().copy(),
                    None if li is None else li["nrej"].cpu().numpy().copy()))
        inner()
    kf._qa_accumulate = spy
    kf.run(grid, *run.args)
    mask = kf.partition.local_mask.reshape(-1)
    assert len(out.seen) >= 2
    seen_bits = 0
    for t, (state, qa_in) in out.seen.items():
        per = [e[1:] for e in log if e[0] == t]
        assert len(per) == per_step, (t, len(per))
        st, nobs, nrej = fold_qa(per)
        N = state.N
        assert np.array_equal(qa_in[0][:N].cpu().numpy(), st)
        if nobs is None:
            assert qa_in[1] is None and qa_in[2] is None
        else:
            assert np.array_equal(qa_in[1][:N].cpu().numpy(), nobs) and np.array_equal(qa_in[2][:N].cpu().numpy(), nrej)
        x, P = state.numpy()
        _, _, _, want, _ = product_blocks(x[:, :N].T, blocks_of(P, 7, N), [None] * 7, Z95, kind=state.kind,
                                          status=st, nobs=nobs, nrej=nrej)
        q = out.product_history[t][1].cpu().numpy()
        assert np.array_equal(q[mask] & 0x0F, want & 0x0F) and np.all(q[~mask] == 255)
        seen_bits |= int(np.bitwise_or.reduce(q[mask]))
        # the fold is not the last analysis alone
        differs = any(not np.array_equal(a[0], st) for a in per)
        assert differs or per_step == 1
    return out, kf, seen_bits


def _cpu_engine_args(seed):
    mask, obs, prior, x0, Pinv, Q = _setup(seed=seed)

    def make(out, **cfg):
        run = lambda kf, grid: kf.run(grid, x0, None, Pinv)       # noqa: E731
        run.args = (x0, None, Pinv)
        return _engine(mask, obs, Q, out=out, **cfg), run
    return make, mask


def test_qa_inputs_fold_over_the_dates_of_a_timestep():
    """A 48-day grid over the 16-day source: 3 dates per timestep, gate on."""
    make, _ = _cpu_engine_args(seed=6)
    grid = _grid(3, step=48)
    _, _, bits = check_qa_fold(make, grid, 3, innovation_gate=1.0)
    assert bits & 8, "the gate rejected nothing: the nobs / nrej sums were not exercised"


def test_qa_inputs_under_band_sequential():
    """One analysis per band: a pixel is without an observation only where every band is."""
    make, mask = _cpu_engine_args(seed=6)
    out, kf, _ = check_qa_fold(make, _grid(4), 2, band_sequential=True)
    ref = k.DeviceOutput(k.TIP_PARAMETERS, keep_history=True, qa=True)
    kf2, run2 = make(ref)
    run2(kf2, _grid(4))
    m = kf.partition.local_mask.reshape(-1)
    for t in ref.product_history:
        a, b = out.product_history[t][1].numpy()[m], ref.product_history[t][1].numpy()[m]
        assert np.array_equal(a & 1, b & 1) and not np.all(a & 1)


GT = [500000., 10., 0., 4000000., 0., -10.]


def check_files(tmp_path, make, encoder, n_dates):
    """KafkaOutput files against the DeviceOutput history, sample for sample; the
    QA file; every standard file byte-identical to the run without the option
    (the default configuration: the information form, whose state and rasters
    do not depend on whether the rasters are fused into the analysis; for the
    gain form see ``check_standard_planes_equal_unfused_run``)."""
    ref = k.DeviceOutput(k.TIP_PARAMETERS, keep_history=True, physical=k.TIP_TRANSFORMS, qa=True)
    kf, run = make(ref)
    run(kf)
    # the run without the option, everything else at its default (conditional uncertainty, the
    # information form, rasters fused into the analysis); the option moves the engine to the unfused launches
    plain = k.KafkaOutput(k.TIP_PARAMETERS, GT, "EPSG:32630", str(tmp_path / "plain"), encoder=encoder)
    kf, run = make(plain)
    run(kf)
    plain.flush()
    out = k.KafkaOutput(k.TIP_PARAMETERS, GT, "EPSG:32630", str(tmp_path / "prod"), encoder=encoder,
                        physical=k.TIP_TRANSFORMS, qa=True)
    kf, run = make(out)
    run(kf)
    out.flush()
    assert len(ref.product_history) == n_dates
    assert len(plain.written) == 14 * n_dates and len(out.written) == (14 + 3 + 1) * n_dates
    for fn in plain.written:
        with open(fn, "rb") as a, open(os.path.join(tmp_path / "prod", os.path.basename(fn)), "rb") as b:
            assert a.read() == b.read(), os.path.basename(fn)
    for ts, (phys, qa) in ref.product_history.items():
        day = ts.strftime("A%Y%j")
        for g, suffix in enumerate(("", "_lo", "_hi")):
            arr, info = k.read_tiff(tmp_path / "prod" / f"TeLAI_phys_{day}{suffix}.tif")
            assert arr.dtype == np.float32
            assert np.array_equal(arr.reshape(-1).view(np.int32), phys[g].cpu().numpy().view(np.int32))
            md = info["metadata"]
            assert md["UNITS"] == "m2/m2" and float(md["LEVEL"]) == 0.95 and "ln(x)" in md["TRANSFORM"]
        arr, info = k.read_tiff(tmp_path / "prod" / f"QA_{day}.tif")
        assert arr.dtype == np.uint8 and np.array_equal(arr.reshape(-1), qa.cpu().numpy())
        for i in range(8):
            assert f"QA_BIT_{i}" in info["metadata"]
        assert "innovation gate" in info["metadata"]["QA_BIT_3"] and info["metadata"]["QA_FILL"] == "255"
    return ref, kf, run


def check_files_u16(tmp_path, make, encoder):
    """uint16 samples: the product's range defaults to the transform's physical
    range; an unbounded transform needs one under the product's name."""
    rg = {p: (-2.0, 8.0) for p in k.TIP_PARAMETERS}
    urg = {p: (0.0, 20.0) for p in k.TIP_PARAMETERS}
    kw = dict(encoder=encoder, sample_type="uint16", ranges=rg, unc_ranges=urg)
    with pytest.raises(ValueError, match="unbounded"):
        k.KafkaOutput(k.TIP_PARAMETERS, GT, "EPSG:32630", str(tmp_path / "bad"),
                      physical={"a_vis": T("identity", name="albedo")}, **kw)
    k.KafkaOutput(k.TIP_PARAMETERS, GT, "EPSG:32630", str(tmp_path / "ok"),
                  physical={"a_vis": T("identity", name="albedo")}, **dict(kw, ranges=dict(rg, albedo=(0.0, 1.0))))
    ref = k.DeviceOutput(k.TIP_PARAMETERS, keep_history=True, physical=k.TIP_TRANSFORMS)
    kf, run = make(ref)
    run(kf)
    out = k.KafkaOutput(k.TIP_PARAMETERS, GT, "EPSG:32630", str(tmp_path / "u16"), physical=k.TIP_TRANSFORMS, **kw)
    kf, run = make(out)
    run(kf)
    out.flush()
    from kafka_inferenceengine_amd.input_output.tiff import read_tiff_scaled
    for ts, (phys, qa) in ref.product_history.items():
        assert qa is None
        for g, suffix in enumerate(("", "_lo", "_hi")):
            fn = tmp_path / "u16" / f"TeLAI_phys_{ts.strftime('A%Y%j')}{suffix}.tif"
            raw, info = k.read_tiff(fn)
            assert raw.dtype == np.uint16 and info["scale"] == pytest.approx(10.0 / 65534, rel=1e-6)
            val, _ = read_tiff_scaled(fn)
            want = phys[g].cpu().numpy()
            ok = ~np.isnan(want)
            # half a step, and the float32 roundings of the quantiser and of the read-back near 10
            assert np.all(np.abs(val.reshape(-1)[ok] - want[ok]) <= 0.5 * info["scale"] + 8 * U * 10.0)
            assert np.all(raw.reshape(-1)[~ok] == 65535)
    assert out.writer_stats()["saturated"]["total"] >= 0


def test_kafka_output_product_files_equal_device_rasters(tmp_path):
    make, mask, grid = _cpu_engine(seed=5)
    check_files(tmp_path, make, "host", n_dates=3)
    check_files_u16(tmp_path, make, "host")


def test_reference_signature_outputs_products(tmp_path):
    """dump_data (the reference API: scipy blocks) against product_blocks."""
    from kafka_inferenceengine_amd.utils.blocks import blocks_to_sparse
    n, N = 3, 12
    A = blocks_of(pack_rows(spd_blocks(n, 1e3, N, 4), N), n, N)
    rng = np.random.default_rng(2)
    x = rng.uniform(0.05, 1.1, (N, n))
    table = {"a": T("neglog", scale=2.0, lo=np.exp(-5.0), hi=1.0, name="LAI", units="m2/m2"), "c": T("linear", scale=90.0)}
    tl = [table["a"], None, table["c"]]
    t = dt.datetime(2017, 1, 1)
    for level in (0.95, 0.5):
        z = k.credible_z(level)
        mem = k.KafkaOutputMemory(["a", "b", "c"], physical=table, level=level, qa=True)
        for P, Pinv, blocks, kind in ((None, blocks_to_sparse(A), A, "precision"),
                                      (blocks_to_sparse(A), blocks_to_sparse(np.linalg.inv(A)), A, "covariance")):
            mem.dump_data(t, x.reshape(-1), P, Pinv, None, n)
            med, lower, upper, qa, _ = product_blocks(x, blocks, tl, z, kind=kind)
            o = mem.output[t]
            for i, name in enumerate(("LAI", "c_phys")):
                assert np.array_equal(o[name], med[:, i]) and np.array_equal(o[name + "_lo"], lower[:, i])
                assert np.array_equal(o[name + "_hi"], upper[:, i])
            assert np.array_equal(o["QA"], qa) and "a" in o and "a_unc" in o
    mask = np.ones((3, 4), bool)
    mask[1, 2] = False
    xs = x[:mask.sum()]
    out = k.KafkaOutput(["a", "b", "c"], None, "", str(tmp_path), asynchronous=False, physical=table, qa=True)
    out.dump_data(t, xs.reshape(-1), None, blocks_to_sparse(A[:mask.sum()]), mask, n)
    med, lower, upper, qa, _ = product_blocks(xs, A[:mask.sum()], tl, Z95, kind="precision")
    day = t.strftime("A%Y%j")
    for vals, suffix in ((med, ""), (lower, "_lo"), (upper, "_hi")):
        arr, info = k.read_tiff(tmp_path / f"LAI_{day}{suffix}.tif")
        assert np.array_equal(arr[mask], vals[:, 0].astype(np.float32)) and arr[1, 2] == 0
        assert info["metadata"]["UNITS"] == "m2/m2"
    arr, _ = k.read_tiff(tmp_path / f"QA_{day}.tif")
    assert arr.dtype == np.uint8 and np.array_equal(arr[mask], qa) and arr[1, 2] == 255
    assert sorted(os.listdir(tmp_path)) == sorted(
        [f"{p}_{day}{s}.tif" for p in "abc" for s in ("", "_unc")]
        + [f"{p}_{day}{s}.tif" for p in ("LAI", "c_phys") for s in ("", "_lo", "_hi")] + [f"QA_{day}.tif"])


def test_smoother_dump_gets_products(tmp_path):
    """SmootherMixin.smooth dumps through dump_state: products for free, no status bits."""
    from test_smoother import mask_with_holes, run_tip, tip_engine
    mask = mask_with_holes((24, 20))
    kf = tip_engine(mask, None, tmp_path / "ck")
    run_tip(kf, mask, 3)
    out = Recording(k.TIP_PARAMETERS, keep_history=True, physical=k.TIP_TRANSFORMS, qa=True)
    kf.smooth(output=out)
    assert len(out.product_history) == 3
    m = kf.partition.local_mask.reshape(-1)
    for t, (phys, qa) in out.product_history.items():
        state, qa_in = out.seen[t]
        assert qa_in is None
        want_p, want_q = product_of_state(kf, state, None, out.products.table(7), out.products.z, 1)
        assert torch.equal(phys.view(torch.int32), want_p.view(torch.int32)) and torch.equal(qa, want_q)
        assert np.all((qa.numpy()[m] & 0x0F) == 0) and np.all(qa.numpy()[~m] == 255)
        # against float64 on the smoothed state
        x, P = state.numpy()
        med, lower, upper, q64, _ = product_blocks(x[:, :state.N].T, blocks_of(P, 7, state.N),
                                                   out.products.table(7), out.products.z, kind=state.kind)
        assert np.allclose(phys.numpy()[0, m], med[:, 0], rtol=1e-5, atol=1e-5)


def test_cli_run_out_physical(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="4")
    r = subprocess.run([sys.executable, "-m", "kafka_inferenceengine_amd", "run", "--sensor", "bhr", "--size", "24",
                        "20", "--steps", "2", "--n-train", "40", "--device", "cpu", "--out", str(tmp_path / "tif"),
                        "--out-physical", "tip", "--out-interval", "0.9", "--out-qa"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["timesteps"] == 2 and rec["finite"]
    files = sorted(os.listdir(tmp_path / "tif"))
    days = sorted({f.split("_A")[1][:7] for f in files})
    assert len(days) == 2
    want = [f"{p}_A{d}{s}.tif" for d in days for p in k.TIP_PARAMETERS for s in ("", "_unc")]
    want += [f"TeLAI_phys_A{d}{s}.tif" for d in days for s in ("", "_lo", "_hi")] + [f"QA_A{d}.tif" for d in days]
    assert files == sorted(want)
    arr, info = k.read_tiff(tmp_path / "tif" / f"TeLAI_phys_A{days[0]}_lo.tif")
    assert float(info["metadata"]["LEVEL"]) == 0.9 and np.isfinite(arr).all() and (arr >= 0).all()
    arr, info = k.read_tiff(tmp_path / "tif" / f"QA_A{days[0]}.tif")
    assert arr.dtype == np.uint8 and "QA_BIT_0" in info["metadata"]
    r = subprocess.run([sys.executable, "-m", "kafka_inferenceengine_amd", "run", "--sensor", "bhr", "--size", "24",
                        "20", "--steps", "1", "--device", "cpu", "--out-interval", "0.9"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode != 0 and "--out-physical" in r.stderr
