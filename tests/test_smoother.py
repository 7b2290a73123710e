"""Fixed-interval (RTS) smoother: ``pixel_smooth`` on the host runner against
float64, the exact identities, the failure rule, the argument checks, and
``LinearKalman.smooth`` against the batch posterior of the whole series, its
outputs, the CLI, two ranks and the refusals.

Kernel truth is ``rts_smooth_blocks`` (NumPy float64) on the float32-rounded
inputs.  The tolerance is not a fixed number: the yardstick is the same
formulas evaluated in NumPy float32 on the same inputs (``smooth_f32``:
``np.linalg.inv`` and matrix products on float32 arrays).  Per (n, kappa,
mask, kind) case the kernel's maximum error against float64 may be at most
4 x that evaluation's maximum error (the margin covers the hardware reciprocal
square root and a different summation order), with a floor of 16 * 2^-24.

Error measures, over every pixel of a case:
  * ``x_s``: |error| / max(|x_a|, |x_s|) of the pixel;
  * ``P_s``: |error_ij| / sqrt(T_ii T_jj) with T = P_a + G (P_s' + P_p) G^T,
    the sum of the recursion's positive semi-definite terms.  The kernel test's
    ``P_s'`` is independent of the filtered state, so the difference
    ``P_s' - P_p`` may cancel or leave ``P_s`` indefinite; T bounds the size of
    what float32 adds up and equals a small multiple of ``P_s`` for the states
    of a real run.
"""
import datetime as dt
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.engine.state import KFState
from kafka_inferenceengine_amd.input_output.checkpoint import CheckpointManager
from kafka_inferenceengine_amd.ops import kernels as K

from test_marginal import blocks_of, pack_rows, spd_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 3, 4, 7, 10)
KINDS = ("precision", "covariance")
U = 2.0 ** -24
FLOOR = 16 * U
SENTINEL = -7.0


def masks_for(n):
    """{name: bit mask}: all, the last parameter alone, two non-adjacent
    parameters (the first and the last; n >= 3), empty."""
    m = {"all": (1 << n) - 1, "last": 1 << (n - 1), "empty": 0}
    if n >= 3:
        m["two"] = 1 | (1 << (n - 1))
    return m


def indices(mask, n):
    return [j for j in range(n) if (mask >> j) & 1]


# ---------------------------------------------------------------- problems
def problem(n, kappa, N, seed, device="cpu", q_pix=False):
    """Inputs of one backward step with ld = N + 3 and a NaN tail in every row."""
    ld = N + 3
    rng = np.random.default_rng(seed + 1)

    def rows(a):
        out = np.full((a.shape[0], ld), np.nan, dtype=np.float32)
        out[:, :N] = a
        return out
    p = dict(n=n, N=N, ld=ld,
             p_a=pack_rows(spd_blocks(n, kappa, N, seed), ld),
             p_next=pack_rows(spd_blocks(n, kappa, N, seed + 7919), ld),
             x_a=rows(rng.standard_normal((n, N))), x_next=rows(rng.standard_normal((n, N))),
             m=rng.uniform(0.8, 1.1, n).astype(np.float32), q=rng.uniform(0.01, 1.0, n).astype(np.float32),
             q_pix=rows(rng.uniform(0.01, 1.0, (n, N))) if q_pix else None)
    p["t"] = {key: torch.from_numpy(p[key]).to(device) for key in ("p_a", "p_next", "x_a", "x_next")}
    p["t"]["q_pix"] = torch.from_numpy(p["q_pix"]).to(device) if q_pix else None
    return p


def run_smooth(p, mask, kind):
    """(x_s [n, ld], P_s rows [nt, ld], status [ld]) as numpy, outputs sentinel-filled before the launch."""
    t, n, ld = p["t"], p["n"], p["ld"]
    dev = t["x_a"].device
    x = torch.full((n, ld), SENTINEL, dtype=torch.float32, device=dev)
    P = torch.full((K.ntri(n), ld), SENTINEL, dtype=torch.float32, device=dev)
    st = torch.full((ld,), 7, dtype=torch.uint8, device=dev)
    K.smooth(n, t["x_a"], t["p_a"], t["x_next"], t["p_next"], x, P, st, kind=kind, prop_mask=mask, m=p["m"], q=p["q"],
             q_pix=t["q_pix"], N=p["N"])
    return x.cpu().numpy(), P.cpu().numpy(), st.cpu().numpy()


def f64_inputs(p):
    n, N = p["n"], p["N"]
    q = p["q"].astype(np.float64) if p["q_pix"] is None else p["q_pix"][:, :N].T.astype(np.float64)
    return (p["x_a"][:, :N].T.astype(np.float64), blocks_of(p["p_a"], n, N), p["x_next"][:, :N].T.astype(np.float64),
            blocks_of(p["p_next"], n, N), p["m"].astype(np.float64), q)


def smooth_f32(x_a, A, x_next, S, J, m, q, kind):
    """The yardstick: the recursion's formulas in NumPy float32."""
    f = np.float32
    x_a, A, x_next, S = x_a.astype(f), A.astype(f), x_next.astype(f), S.astype(f)
    N, n = x_a.shape
    P_a = np.linalg.inv(A) if kind == "precision" else A
    assert P_a.dtype == f
    if not J:
        return x_a, P_a
    mJ = np.asarray(m, dtype=f)[J]
    qJ = np.broadcast_to(np.asarray(q, dtype=f), (N, n))[:, J]
    x_p = x_a[:, J] * mJ
    P_p = P_a[:, J][:, :, J] * mJ[:, None] * mJ[None, :]
    P_p[:, np.arange(len(J)), np.arange(len(J))] += qJ
    G = (P_a[:, :, J] * mJ[None, None, :]) @ np.linalg.inv(P_p)
    x_s = x_a + (G @ (x_next[:, J] - x_p)[:, :, None])[:, :, 0]
    P_s = P_a + G @ (S[:, J][:, :, J] - P_p) @ G.transpose(0, 2, 1)
    assert x_s.dtype == f and P_s.dtype == f
    return x_s, P_s


def scales(x_a, A, S, J, m, q, kind, x_s):
    """(x scale [N], P scale [N, n, n]) of the error measures (module docstring), float64."""
    N, n = x_a.shape
    P_a = np.linalg.inv(A) if kind == "precision" else A
    T = P_a.copy()
    if J:
        mJ = np.asarray(m)[J]
        qJ = np.broadcast_to(np.asarray(q), (N, n))[:, J]
        P_p = P_a[:, J][:, :, J] * mJ[:, None] * mJ[None, :]
        P_p[:, np.arange(len(J)), np.arange(len(J))] += qJ
        G = (P_a[:, :, J] * mJ[None, None, :]) @ np.linalg.inv(P_p)
        T = T + G @ (S[:, J][:, :, J] + P_p) @ G.transpose(0, 2, 1)
    d = np.sqrt(np.diagonal(T, axis1=1, axis2=2))
    return np.maximum(np.abs(x_a).max(1), np.abs(x_s).max(1)), d[:, :, None] * d[:, None, :]


def errors(x, P, x_t, P_t, sx, sP):
    return float(np.max(np.abs(x - x_t) / sx[:, None])), float(np.max(np.abs(P - P_t) / sP))


def kernel_bound(inputs, J, kind, result_scale=False):
    """(truth x_s, truth P_s, x scale, P scale, x bound, P bound) of one case:
    4 x the float32 evaluation's maximum error, floor 16 * 2^-24.
    ``result_scale``: measure P_s relative to sqrt(P_s,ii P_s,jj) of the truth
    itself -- for the states of a run, whose smoothed covariance is SPD."""
    x_a, A, x_n, S, m, q = inputs
    x_t, P_t = k.rts_smooth_blocks(x_a, A, x_n, S, J, m, q, kind)
    sx, sP = scales(x_a, A, S, J, m, q, kind, x_t)
    if result_scale:
        d = np.sqrt(np.diagonal(P_t, axis1=1, axis2=2))
        sP = d[:, :, None] * d[:, None, :]
    x32, P32 = smooth_f32(x_a, A, x_n, S, J, m, q, kind)
    ex, eP = errors(x32.astype(np.float64), P32.astype(np.float64), x_t, P_t, sx, sP)
    return x_t, P_t, sx, sP, max(4 * ex, FLOOR), max(4 * eP, FLOOR)


def check_kernel(n, kappa, N, seed, device="cpu", q_pix=False, masks=None):
    """Every mask and both kinds of one problem against float64; the layout
    (sentinel past N), the status, and the exact identities."""
    p = problem(n, kappa, N, seed, device, q_pix)
    inputs = f64_inputs(p)
    for name, mask in masks_for(n).items():
        if masks is not None and name not in masks:
            continue
        J = indices(mask, n)
        for kind in KINDS:
            x, P, st = run_smooth(p, mask, kind)
            assert np.all(x[:, N:] == SENTINEL) and np.all(P[:, N:] == SENTINEL) and np.all(st[N:] == 7)
            assert np.all(st[:N] == 0), (name, kind, np.flatnonzero(st[:N]))
            x_t, P_t, sx, sP, bx, bP = kernel_bound(inputs, J, kind)
            ex, eP = errors(x[:, :N].T.astype(np.float64), blocks_of(P, n, N), x_t, P_t, sx, sP)
            print(f"n={n} kappa={kappa:g} N={N} mask={name} {kind}{' q_pix' if q_pix else ''}: "
                  f"x err/bound {ex / bx:.3f} P err/bound {eP / bP:.3f} (bounds {bx / U:.1f} u, {bP / U:.1f} u)")
            assert ex <= bx and eP <= bP, (name, kind, ex, bx, eP, bP)
            if not J:
                # nothing links the steps: the filtered moments, bit for bit
                assert np.array_equal(x[:, :N], p["x_a"][:, :N])
                if kind == "covariance":
                    assert np.array_equal(P[:, :N], p["p_a"][:, :N])
            if len(J) == 1 and kind == "precision":
                check_single_parameter_identity(p, inputs, J[0], P, P_t, sP, bP)


def check_single_parameter_identity(p, inputs, j, P, P_t, sP, bP):
    """One propagated parameter j: P_s^-1 differs from the filtered precision L
    in entry (j, j) only.  The float64 inverse of the kernel's P_s against L
    outside (j, j), within the kernel-test bound carried through the inverse:
    the truth's inverse has the identity exactly, and for the kernel's
    P_k = P_s + E,  inv(P_k) - inv(P_s) = -inv(P_s) E inv(P_k)  exactly.  The
    kernel test bounds |E_ab| by bP t_a t_b (t = sqrt(diag T), its P measure),
    so entry (i, k) may deviate by at most  bP (|inv P_s| t)_i (|inv P_k| t)_k."""
    n, N = p["n"], p["N"]
    A = inputs[1]
    if n == 1:
        return
    t = np.sqrt(np.diagonal(sP, axis1=1, axis2=2))
    Pk = blocks_of(P, n, N)
    Ls, Lk = np.linalg.inv(P_t), np.linalg.inv(Pk)
    off = np.ones((n, n), bool)
    off[j, j] = False
    assert np.max(np.abs(Ls - A)[:, off] / np.abs(A).max()) < 1e-9        # the identity itself, float64
    bound = bP * np.einsum("pia,pa->pi", np.abs(Ls), t)[:, :, None] * np.einsum("pkb,pb->pk", np.abs(Lk), t)[:, None, :]
    ratio = float(np.max((np.abs(Lk - A) / (bound + 1e-9 * np.abs(A).max()))[:, off]))
    print(f"   single parameter {j}: inverse off-(j, j) deviation / bound {ratio:.3f}")
    assert ratio <= 1.0


def check_failure_rule(n, N, seed, device="cpu"):
    """A -I block, a NaN in the filtered rows, a NaN in P_s': status 1 on that
    pixel alone, x_s = x_a, P_s = P_a where the filtered block is SPD and NaN
    rows otherwise, every other pixel as in the clean run bit for bit."""
    iu = np.triu_indices(n)
    diag_rows = np.nonzero(iu[0] == iu[1])[0]
    mask = (1 << n) - 1
    for kind in KINDS:
        clean = run_smooth(problem(n, 1e3, N, seed, device), mask, kind)
        p_a = run_smooth(problem(n, 1e3, N, seed, device), 0, kind)[1]
        for case in ("minus_identity", "nan_filtered", "nan_next"):
            p = problem(n, 1e3, N, seed, device)
            bad = N // 2
            if case == "minus_identity":
                p["t"]["p_a"][:, bad] = 0.0
                p["t"]["p_a"][diag_rows, bad] = -1.0
            elif case == "nan_filtered":
                p["t"]["p_a"][K.ntri(n) - 1 if n == 1 else 1, bad] = float("nan")
            else:
                p["t"]["p_next"][0, bad] = float("nan")
            x, P, st = run_smooth(p, mask, kind)
            others = np.delete(np.arange(N), bad)
            assert st[bad] == 1 and np.all(st[others] == 0), (case, kind)
            assert np.array_equal(x[:, bad], p["x_a"][:, bad])
            if case == "nan_next":
                # the filtered block is SPD: P_a as the kernel forms it (the empty mask's output)
                assert np.array_equal(P[:, bad], p_a[:, bad])
                if kind == "covariance":
                    assert np.array_equal(P[:, bad], p["p_a"][:, bad])
            else:
                assert np.isnan(P[:, bad]).all()
            for got, ref in zip((x, P), clean[:2]):
                assert np.array_equal(got[:, others], ref[:, others]), (case, kind)


# ------------------------------------------------------------ kernel tests
@pytest.mark.parametrize("kappa", [10.0, 1e3])
@pytest.mark.parametrize("n", SIZES)
def test_smooth_host_runner_against_float64(n, kappa):
    check_kernel(n, kappa, 257, seed=100 * n + int(np.log10(kappa)))


@pytest.mark.parametrize("n", SIZES)
def test_smooth_host_runner_per_pixel_q(n):
    check_kernel(n, 1e3, 131, seed=50 + n, q_pix=True)


@pytest.mark.parametrize("n", SIZES)
def test_smooth_failure_rule(n):
    check_failure_rule(n, 67, seed=n)


def test_smooth_argument_checks():
    p = problem(3, 10.0, 20, 0)
    t = p["t"]
    x, P, st = torch.zeros((3, 23)), torch.zeros((6, 23)), torch.zeros(23, dtype=torch.uint8)
    kw = dict(kind="precision", prop_mask=7, m=p["m"], q=p["q"], N=20)
    K.smooth(3, t["x_a"], t["p_a"], t["x_next"], t["p_next"], x, P, st, **kw)
    with pytest.raises(ValueError):
        K.smooth(3, t["x_a"], t["p_a"], t["x_next"], t["p_next"], x, P, st, **dict(kw, kind="variance"))
    with pytest.raises(ValueError):
        K.smooth(3, t["x_a"], t["p_a"], t["x_next"], t["p_next"], x, P, st, **dict(kw, prop_mask=8))
    with pytest.raises(ValueError):
        K.smooth(5, t["x_a"], t["p_a"], t["x_next"], t["p_next"], x, P, st, **kw)
    with pytest.raises(ValueError):
        K.smooth(3, t["x_a"], t["p_a"][:5], t["x_next"], t["p_next"], x, P, st, **kw)
    with pytest.raises(ValueError):
        K.smooth(3, t["x_a"], t["p_a"], t["x_next"], t["p_next"][:5], x, P, st, **kw)
    with pytest.raises(ValueError):
        K.smooth(3, t["x_a"], t["p_a"], t["x_next"], t["p_next"], x, P, st[:10], **kw)
    with pytest.raises(TypeError):
        K.smooth(3, t["x_a"], t["p_a"].double(), t["x_next"], t["p_next"], x, P, st, **kw)
    with pytest.raises(TypeError):
        K.smooth(3, t["x_a"], t["p_a"], t["x_next"].double(), t["p_next"], x, P, st, **kw)


def test_rts_smooth_blocks_equals_batch_solve():
    """The oracle itself: with every parameter propagated, the chain of backward
    steps over a filtered series equals the batch posterior (n = 4, 5 steps)."""
    rng = np.random.default_rng(3)
    n, T, N = 4, 5, 6
    m, q = rng.uniform(0.8, 1.1, n), rng.uniform(0.05, 0.5, n)
    L0 = spd_blocks(n, 10.0, N, 1)
    x0 = rng.standard_normal((N, n))
    W = rng.uniform(0.0, 3.0, (T, N, n)) * (rng.random((T, N, 1)) > 0.3)
    Y = rng.standard_normal((T, N, n))
    xf, Pf = x0, np.linalg.inv(L0)
    filt = []
    for t in range(T):
        if t:
            xf, Pf = filt[-1][0] * m, filt[-1][1] * m[:, None] * m[None, :] + np.diag(q)
        La = np.linalg.inv(Pf) + np.einsum("pi,ij->pij", W[t], np.eye(n))
        Pa = np.linalg.inv(La)
        xa = np.einsum("pij,pj->pi", Pa, np.einsum("pij,pj->pi", np.linalg.inv(Pf), xf) + W[t] * Y[t])
        filt.append((xa, Pa))
    xs, Ps = filt[-1]
    sm = [(xs, Ps)]
    for t in range(T - 2, -1, -1):
        xs, Ps = k.rts_smooth_blocks(filt[t][0], filt[t][1], xs, Ps, (1 << n) - 1, m, q, "covariance")
        sm.append((xs, Ps))
    sm.reverse()
    xb, Pb = batch_posterior(x0, L0, W, Y, m, q)
    for t in range(T):
        assert np.allclose(sm[t][0], xb[t], rtol=0, atol=1e-12) and np.allclose(sm[t][1], Pb[t], rtol=0, atol=1e-12)
    # a partial J embedded in n x n (unit diagonal outside J, zero gain columns) equals the J-block form
    J = [1, 3]
    a = k.rts_smooth_blocks(filt[0][0], filt[0][1], sm[1][0], sm[1][1], J, m, q, "covariance")
    b = k.rts_smooth_blocks(filt[0][0], np.linalg.inv(filt[0][1]), sm[1][0], sm[1][1], (1 << 1) | (1 << 3), m, q)
    assert np.allclose(a[0], b[0], atol=1e-12) and np.allclose(a[1], b[1], atol=1e-12)


def batch_posterior(x0, L0, W, Y, m, q):
    """Float64 batch solution per pixel of T steps with identity observations:
    the (T n)^2 precision from the initial forecast (x0, L0), the observation
    terms diag(W[t]) (values Y[t]) and the Q^-1 transition terms, inverted.
    Returns (means [T, N, n], covariance blocks [T, N, n, n])."""
    T, N, n = W.shape
    q = np.broadcast_to(np.asarray(q, dtype=np.float64), (N, n))
    m = np.asarray(m, dtype=np.float64)
    A = np.zeros((N, T * n, T * n))
    b = np.zeros((N, T * n))
    A[:, :n, :n] += L0
    b[:, :n] += np.einsum("pij,pj->pi", L0, x0)
    ar = np.arange(n)
    for t in range(T):
        s = t * n
        A[:, s + ar, s + ar] += W[t]
        b[:, s:s + n] += W[t] * Y[t]
        if t + 1 < T:
            qi = 1.0 / q
            A[:, s + ar, s + ar] += m * qi * m
            A[:, s + n + ar, s + n + ar] += qi
            A[:, s + ar, s + n + ar] -= m * qi
            A[:, s + n + ar, s + ar] -= m * qi
    C = np.linalg.inv(A)
    x = np.einsum("pij,pj->pi", C, b)
    return (np.stack([x[:, t * n:(t + 1) * n] for t in range(T)]),
            np.stack([C[:, t * n:(t + 1) * n, t * n:(t + 1) * n] for t in range(T)]))


# ------------------------------------------------------------------ engine
class StateLog:
    """An output that keeps every dumped state (``dump_state`` protocol)."""

    uncertainty = "conditional"

    def __init__(self):
        self.states = {}

    def dump_state(self, timestep, state, engine):
        self.states[timestep] = state.clone()


def mask_with_holes(shape):
    mask = np.ones(shape, bool)
    mask[::7, 3::5] = False
    mask[:3, :4] = False
    return mask


def _grid(n, step=16, start=dt.datetime(2017, 1, 1)):
    return [start + dt.timedelta(days=step * i) for i in range(n)]


def load_filtered(kf, root):
    """[(timestep, KFState)] of the run's committed checkpoints."""
    return [(t, CheckpointManager.load(p, kf)[0]) for t, p in CheckpointManager.committed(root)]


def cov_blocks(st):
    """(x [N, n], P blocks [N, n, n]) in float64 of a state of either kind."""
    x, P = st.numpy()
    B = blocks_of(P, x.shape[0], st.N)
    return x.T.astype(np.float64), (np.linalg.inv(B) if st.kind == "precision" else B)


def measure(x, P, x_t, P_t):
    d = np.sqrt(np.diagonal(P_t, axis1=1, axis2=2))
    return errors(x, P, x_t, P_t, np.maximum(np.abs(x_t).max(1), 1e-30), d[:, :, None] * d[:, None, :])


def chain_bound(filt, mask, m, q, n):
    """The kernel-test bound over a run's own filtered states: per backward step
    4 x the float32 evaluation's error against ``rts_smooth_blocks`` (floor
    16 * 2^-24), the maximum over the steps, P_s measured relative to
    sqrt(P_s,ii P_s,jj); and the float64 chain itself."""
    J = indices(mask, n)
    x_s, P_s = cov_blocks(filt[-1][1])
    chain = [(x_s, P_s)]
    bx = bP = FLOOR
    for _, st in reversed(filt[:-1]):
        x, P = st.numpy()
        x_a, A = x.T.astype(np.float64), blocks_of(P, n, st.N)
        x_t, P_t, sx, sP, b1, b2 = kernel_bound((x_a, A, x_s, P_s, m, q), J, st.kind, result_scale=True)
        bx, bP = max(bx, b1), max(bP, b2)
        x_s, P_s = x_t, P_t
        chain.append((x_s, P_s))
    chain.reverse()
    return chain, bx, bP


def check_engine_against_batch(tmp_path, form, device="cpu"):
    """Identity observations, every q > 0, the exact propagator of the form:
    every step's smoothed mean and covariance against the float64 batch
    posterior of the whole series.

    Tolerance: the forward filter's own error against the batch solution at the
    last step (the smoother changes nothing there) times the number of steps,
    plus the kernel-test bound over the run's states."""
    mask = mask_with_holes((24, 20))
    grid = _grid(6)
    dates = [g + dt.timedelta(days=1) for g in grid[:5]]
    obs = k.SyntheticIdentityObservations(mask, dates=dates, device=device, stream=False, n_pool=5, field_cell=8,
                                          encoding="f32", cloud_fraction=0.35, seed=4)
    prior = k.JRCPrior(k.TIP_PARAMETERS, mask)
    x0, Pinv = prior.process_prior(None)
    n, T = 7, 5
    q = 0.05 * np.diag(np.linalg.inv(np.asarray(prior.device_prior(None).cinv, dtype=np.float64)))
    prop = k.propagate_standard_kalman if form == "gain" else k.propagate_information_filter_SLOW
    kf = k.LinearKalman(obs, None, mask, k.create_linear_observation_operator, k.TIP_PARAMETERS,
                        state_propagation=prop, device=device,
                        config=k.EngineConfig(analysis_form=form, checkpoint_dir=str(tmp_path / "ck"),
                                              checkpoint_every=1))
    kf.set_trajectory_model()
    kf.set_trajectory_uncertainty(q)
    kf.run(grid, x0, None, Pinv)
    log = StateLog()
    first, recs = kf.smooth(output=log)
    assert [r["timestep"] for r in recs] == [g.isoformat() for g in grid[1:]]
    assert all(r["fallback_pixels"] == 0 for r in recs)
    filt = load_filtered(kf, tmp_path / "ck")
    assert [t for t, _ in filt] == grid[1:] == sorted(log.states)
    assert all(s.kind == "covariance" for s in log.states.values())
    assert torch.equal(first.x, log.states[grid[1]].x) and torch.equal(first.P, log.states[grid[1]].P)
    # last step: the filtered state converted by the engine's own _as_kind
    last = kf._as_kind(filt[-1][1], "covariance")
    assert torch.equal(log.states[grid[-1]].x, last.x) and torch.equal(log.states[grid[-1]].P, last.P)

    # the batch posterior from what the filter saw
    N = kf.N
    W = np.zeros((T, N, n))
    Y = np.zeros((T, N, n))
    for t, d in enumerate(dates):
        for b in range(n):
            y, w = obs.get_device_band_data(d, b).decode()
            Y[t, :, b], W[t, :, b] = y.cpu().numpy()[:N], w.cpu().numpy()[:N]
    st0 = kf.initial_state(x0, None, Pinv)
    x0b, P0 = cov_blocks(st0)
    xb, Pb = batch_posterior(x0b, np.linalg.inv(P0), W, Y, np.ones(n), q.astype(np.float32).astype(np.float64))
    e_fx, e_fP = measure(*cov_blocks(filt[-1][1]), xb[-1], Pb[-1])
    _, bx, bP = chain_bound(filt, (1 << n) - 1, np.ones(n), q.astype(np.float32).astype(np.float64), n)
    tol_x, tol_P = T * e_fx + bx, T * e_fP + bP
    print(f"{form}: filter error at the last step x {e_fx / U:.1f} u, P {e_fP / U:.1f} u; kernel bound x {bx / U:.1f} u, "
          f"P {bP / U:.1f} u; tolerance x {tol_x / U:.1f} u, P {tol_P / U:.1f} u")
    observed = W.max(axis=2) > 0
    assert (~observed).any(axis=1).all() and observed.any(axis=1).all()
    for t in range(T):
        xs, Ps = cov_blocks(log.states[grid[t + 1]])
        ex, eP = measure(xs, Ps, xb[t], Pb[t])
        print(f"   step {t}: x err/tol {ex / tol_x:.3f}, P err/tol {eP / tol_P:.3f}")
        assert ex <= tol_x and eP <= tol_P, (t, ex, tol_x, eP, tol_P)
        _, Pa = cov_blocks(filt[t][1])
        ds, da = np.diagonal(Ps, axis1=1, axis2=2), np.diagonal(Pa, axis1=1, axis2=2)
        assert np.all(ds <= da * (1 + bP))
        if t + 1 < T:
            gap = ~observed[t] & observed[t + 1]
            assert gap.any()
            assert np.all(ds[gap] < da[gap])
    return kf, log, filt


@pytest.mark.parametrize("form", ["information", "gain"])
def test_engine_smooth_equals_batch_posterior(tmp_path, form):
    check_engine_against_batch(tmp_path, form)


def tip_engine(mask, out, ckdir, device="cpu", n_train=60, comm=None, partition=None, **cfg):
    kw = dict(partition=partition) if partition is not None else {}
    obs = k.SyntheticBHRObservations(mask, n_train=n_train, device=device, stream=False, n_pool=2, seed=1, **kw)
    kf = k.LinearKalman(obs, out, mask, k.create_nonlinear_observation_operator, k.TIP_PARAMETERS,
                        state_propagation=k.propagate_information_filter_LAI, device=device, comm=comm,
                        partition=partition,
                        config=k.EngineConfig(checkpoint_dir=None if ckdir is None else str(ckdir),
                                              checkpoint_every=1 if ckdir is not None else 0, **cfg))
    kf.set_trajectory_uncertainty(np.array([0, 0, 0, 0, 0, 0, 0.04]))
    return kf


def run_tip(kf, mask, steps):
    st = kf.run(_grid(steps + 1), kf.state_from_prior(k.JRCPrior(k.TIP_PARAMETERS, mask)), None, None)
    if kf.device.type == "cuda":
        torch.cuda.synchronize()
    return st


def check_engine_headline(tmp_path, device="cpu", shape=(40, 33), steps=4):
    """JRC-TIP with the LAI propagator (J = {6}): the smoothed states against
    ``rts_smooth_blocks`` over the run's own checkpointed states."""
    mask = mask_with_holes(shape)
    kf = tip_engine(mask, None, tmp_path / "ck", device)
    run_tip(kf, mask, steps)
    log, hist = StateLog(), k.DeviceOutput(k.TIP_PARAMETERS, keep_history=True)
    _, recs = kf.smooth(output=log)
    _, recs2 = kf.smooth(output=hist)
    assert [r["fallback_pixels"] for r in recs] == [0] * steps == [r["fallback_pixels"] for r in recs2]
    assert sorted(hist.history) == sorted(log.states) and len(hist.history) == steps
    filt = load_filtered(kf, tmp_path / "ck")
    n = 7
    chain, bx, bP = chain_bound(filt, 1 << 6, np.ones(n), np.array([0, 0, 0, 0, 0, 0, 0.04], np.float32).astype(float), n)
    for t, (ts, st) in enumerate(filt):
        sm = log.states[ts]
        xs, Ps = cov_blocks(sm)
        if t == steps - 1:
            last = kf._as_kind(st, "covariance")
            assert torch.equal(sm.x, last.x) and torch.equal(sm.P, last.P)
        else:
            # each step against the oracle applied to the kernel's own next state: one kernel error per step
            nx, nP = cov_blocks(log.states[filt[t + 1][0]])
            x, P = st.numpy()
            x_t, P_t, sx, sP, b1, b2 = kernel_bound((x.T.astype(np.float64), blocks_of(P, n, st.N), nx, nP, np.ones(n),
                                                     np.array([0, 0, 0, 0, 0, 0, 0.04], np.float32).astype(float)),
                                                    [6], st.kind, result_scale=True)
            ex, eP = errors(xs, Ps, x_t, P_t, sx, sP)
            print(f"   step {t}: x err/bound {ex / b1:.3f}, P err/bound {eP / b2:.3f}")
            assert ex <= b1 and eP <= b2
        if t < steps - 1:
            # (the last step is the filtered state itself, asserted above)
            _, Pa = cov_blocks(st)
            assert np.all(Ps[:, 6, 6] <= Pa[:, 6, 6] * (1 + bP))
        # the rasters: the smoothed mean on the state mask
        m = hist.history[ts][0].cpu().numpy()[:, kf.partition.local_mask.reshape(-1)]
        assert np.array_equal(m, sm.x[:, :sm.N].cpu().numpy())
    return kf


def test_engine_smooth_tip_lai_host(tmp_path):
    check_engine_headline(tmp_path, shape=(24, 20), steps=3)


def check_outputs(tmp_path, device="cpu", shape=(24, 20), steps=3):
    """KafkaOutput (host encoder) files of a smoothed run equal the DeviceOutput
    rasters, with and without marginal uncertainty."""
    mask = mask_with_holes(shape)
    kf = tip_engine(mask, None, tmp_path / "ck", device)
    run_tip(kf, mask, steps)
    for unc in ("conditional", "marginal"):
        ref = k.DeviceOutput(k.TIP_PARAMETERS, keep_history=True, uncertainty=unc)
        kf.smooth(output=ref)
        out = k.KafkaOutput(k.TIP_PARAMETERS, [500000., 10., 0., 4000000., 0., -10.], "EPSG:32630",
                            str(tmp_path / unc), uncertainty=unc, encoder="host")
        kf.smooth(output=out)
        out.flush()
        assert len(out.written) == 14 * steps == 14 * len(ref.history)
        for ts, (m, u) in ref.history.items():
            for p, name in enumerate(k.TIP_PARAMETERS):
                core = f"{name}_{ts.strftime('A%Y%j')}"
                arr, _ = k.read_tiff(tmp_path / unc / f"{core}.tif")
                assert np.array_equal(arr.reshape(-1), m[p].cpu().numpy())
                arr, info = k.read_tiff(tmp_path / unc / f"{core}_unc.tif")
                assert np.array_equal(arr.reshape(-1), u[p].cpu().numpy())
                assert info.get("uncertainty") == ("marginal" if unc == "marginal" else None)


def test_smoothed_output_files_equal_device_rasters(tmp_path):
    check_outputs(tmp_path)


def test_smooth_from_states_and_empty_link(tmp_path):
    """An explicit list of states gives what the checkpoints give; a propagator
    that carries nothing (reset to the prior) returns the filtered states."""
    mask = mask_with_holes((24, 20))
    kf = tip_engine(mask, None, tmp_path / "ck")
    run_tip(kf, mask, 3)
    a, b = StateLog(), StateLog()
    kf.smooth(output=a)
    filt = load_filtered(kf, tmp_path / "ck")
    first, recs = kf.smooth(states=list(reversed(filt)), output=b)
    assert len(recs) == 3 and sorted(a.states) == sorted(b.states)
    for ts in a.states:
        assert torch.equal(a.states[ts].x, b.states[ts].x) and torch.equal(a.states[ts].P, b.states[ts].P)
    assert not torch.equal(first.x, filt[0][1].x)
    obs = k.SyntheticBHRObservations(mask, n_train=60, device="cpu", stream=False, n_pool=2, seed=1)
    kf0 = k.LinearKalman(obs, None, mask, k.create_nonlinear_observation_operator, k.TIP_PARAMETERS,
                         state_propagation=k.no_propagation, device="cpu")
    c = StateLog()
    first, recs = kf0.smooth(states=filt, output=c)
    assert [r["fallback_pixels"] for r in recs] == [0, 0, 0]
    for ts, st in filt:
        assert torch.equal(c.states[ts].x, st.x) and torch.equal(c.states[ts].P, st.P)
    assert torch.equal(first.x, filt[0][1].x)


def test_smooth_refusals(tmp_path):
    mask = mask_with_holes((24, 20))
    kf = tip_engine(mask, None, tmp_path / "ck")
    run_tip(kf, mask, 3)
    # a missing checkpoint, named
    gone = CheckpointManager.committed(tmp_path / "ck")[1]
    (gone[1] / "manifest.json").unlink()
    with pytest.raises(FileNotFoundError, match=gone[0].isoformat()):
        kf.smooth()
    with pytest.raises(ValueError, match="checkpoint"):
        tip_engine(mask, None, None).smooth()
    filt = [(dt.datetime(2017, 1, 17), KFState.empty(7, int(mask.sum()), torch.device("cpu")))]
    # the spatial prior
    with pytest.raises(ValueError, match="spatial"):
        tip_engine(mask, None, None, spatial_gamma=50.0, spatial_params=[6], jacobi_sweeps=4).smooth(states=filt)
    # a prior blended with a propagator
    obs = k.SyntheticBHRObservations(mask, n_train=60, device="cpu", stream=False, n_pool=2, seed=1)
    kfb = k.LinearKalman(obs, None, mask, k.create_nonlinear_observation_operator, k.TIP_PARAMETERS,
                         state_propagation=k.propagate_information_filter_LAI,
                         prior=k.JRCPrior(k.TIP_PARAMETERS, mask), device="cpu")
    with pytest.raises(ValueError, match="blend"):
        kfb.smooth(states=filt)
    # a propagator without a device_spec

    def user_prop(*a, **kw):
        return k.propagate_information_filter_LAI(*a, **kw)
    kfu = k.LinearKalman(obs, None, mask, k.create_nonlinear_observation_operator, k.TIP_PARAMETERS,
                         state_propagation=user_prop, device="cpu")
    with pytest.raises(ValueError, match="device_spec"):
        kfu.smooth(states=filt)


def test_cli_run_smooth_out(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="4")
    r = subprocess.run([sys.executable, "-m", "kafka_inferenceengine_amd", "run", "--sensor", "bhr", "--size", "24",
                        "20", "--steps", "3", "--n-train", "40", "--device", "cpu", "--out", str(tmp_path / "tif"),
                        "--smooth-out", str(tmp_path / "smooth")], capture_output=True, text=True, timeout=600, env=env,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["timesteps"] == 3 and rec["finite"]
    assert rec["smooth"]["fallback_pixels"] == [0, 0, 0] and len(rec["smooth"]["timesteps"]) == 3
    fwd = sorted(f for f in os.listdir(tmp_path / "tif") if f.endswith(".tif"))
    sm = sorted(f for f in os.listdir(tmp_path / "smooth") if f.endswith(".tif"))
    assert fwd == sm and len(sm) == 3 * 2 * 7
    assert len(CheckpointManager.committed(tmp_path / "smooth" / "checkpoints")) == 3
    lai = sorted(f for f in sm if f.startswith("TeLAI") and not f.endswith("_unc.tif"))
    first, last = lai[0], lai[-1]
    assert np.array_equal(k.read_tiff(tmp_path / "tif" / last)[0], k.read_tiff(tmp_path / "smooth" / last)[0])
    assert not np.array_equal(k.read_tiff(tmp_path / "tif" / first)[0], k.read_tiff(tmp_path / "smooth" / first)[0])


# ------------------------------------------------------------------ 2 ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_run(world, rank, ckdir, q):
    from kafka_inferenceengine_amd.parallel import Comm, StripPartition

    if world > 1:
        torch.set_num_threads(1)
    mask = mask_with_holes((30, 22))
    comm = Comm(rank, world, "cpu") if world > 1 else Comm.single("cpu")
    part = StripPartition(mask, rank, world)
    kf = tip_engine(mask, None, ckdir, comm=comm, partition=part)
    run_tip(kf, mask, 3)
    log = StateLog()
    _, recs = kf.smooth(output=log)
    ts = sorted(log.states)
    q.put((rank, np.stack([log.states[t].x[:, :kf.N].numpy() for t in ts]),
           np.stack([log.states[t].P[:, :kf.N].numpy() for t in ts]), [r["fallback_pixels"] for r in recs]))


def _rank_worker(rank, world, port, ckdir, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _rank_run(world, rank, ckdir, q)
    finally:
        dist.destroy_process_group()


def test_smooth_two_ranks_equal_one_rank(tmp_path):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    _rank_run(1, 0, str(tmp_path / "one"), q)
    one = q.get()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, str(tmp_path / "two"), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=300) for _ in range(2)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert np.array_equal(np.concatenate([r[1] for r in res], 2), one[1])
    assert np.array_equal(np.concatenate([r[2] for r in res], 2), one[2])
    assert all(r[3] == [0, 0, 0] for r in res) and one[3] == [0, 0, 0]
