"""State propagation, prior blending and Hessian corrections — reference API.

Signatures follow ``kafka/inference/kf_tools.py`` so a reference user can swap
imports; the bodies operate on per-pixel blocks (vectorised NumPy, float64)
instead of global SuperLU solves.  Every propagator carries a ``device_spec``
(mode + parameters of the gfx950 propagate kernel, ``csrc/kf_core.h``
``pixel_propagate``) that the engine uses on its device path.
"""
from __future__ import annotations

import logging
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp

from ..models.operators import band_selecta
from ..models.priors import tip_prior
from ..utils.blocks import blocks_to_sparse, sparse_to_blocks

LOG = logging.getLogger(__name__)

# keep in sync with csrc/kf_core.h PropMode
PROP_PRIOR, PROP_PRIOR_PARTIAL, PROP_INFO_APPROX, PROP_INFO_EXACT, PROP_STANDARD, PROP_IDENTITY = range(6)


class NoHessianMethod(Exception):
    """Forward model cannot provide a Hessian (kf_tools.py:13-17)."""

    def __init__(self, message):
        super().__init__(message)
        self.message = message


@dataclass
class PropagatorSpec:
    """Device description of a propagator."""
    mode: int
    output: str = "precision"                    # 'precision' | 'covariance'
    propagated: tuple = ()                       # PROP_PRIOR_PARTIAL
    reset_mean: np.ndarray | None = None         # PROP_PRIOR / PROP_PRIOR_PARTIAL
    reset_cinv: np.ndarray | None = None
    extra: dict = field(default_factory=dict)


def _diag(m, n_total=None):
    if m is None:
        return None
    if sp.issparse(m):
        return np.asarray(m.diagonal())
    m = np.asarray(m)
    return np.diag(m) if m.ndim == 2 else m


def _apply_M(M_matrix, x):
    if M_matrix is None:
        return np.asarray(x) * 1.0
    return np.asarray(M_matrix.dot(x)).ravel() if hasattr(M_matrix, "dot") else np.asarray(M_matrix) @ x


# ------------------------------------------------------------------ priors
def tip_prior_noLAI(prior):
    """Tiled TIP prior without LAI information (the reference called
    ``tip_prior`` with the wrong arity, kf_tools.py:118-120)."""
    return tip_prior_full(prior)


def tip_prior_full(prior):
    """TIP prior tiled over ``prior['n_pixels']`` (kf_tools.py:123-133)."""
    x_prior, _, c_inv_prior = tip_prior()
    n_pixels = int(prior["n_pixels"])
    mean = np.tile(x_prior, n_pixels)
    blocks = np.broadcast_to(c_inv_prior.astype(np.float32), (n_pixels, 7, 7))
    return mean, blocks_to_sparse(np.ascontiguousarray(blocks), "csr", np.float32)


def blend_prior(prior_mean, prior_cov_inverse, x_forecast, P_forecast_inverse, quirk: bool = True,
                n_params: int | None = None):
    """Gaussian product of prior and forecast (kf_tools.py:75-96).

    The reference swaps the operands of the right-hand side
    (``b = P_f^-1 mu + C^-1 x_f``); ``quirk=True`` (the reference-API default)
    reproduces that, ``quirk=False`` is the textbook product."""
    combined = P_forecast_inverse + prior_cov_inverse
    if quirk:
        b = P_forecast_inverse.dot(prior_mean) + prior_cov_inverse.dot(x_forecast)
    else:
        b = P_forecast_inverse.dot(x_forecast) + prior_cov_inverse.dot(prior_mean)
    b = np.asarray(b, dtype=np.float32).astype(np.float64)
    n = n_params or _guess_block(combined, len(b))
    blocks = sparse_to_blocks(combined, n, check=False).astype(np.float32).astype(np.float64)
    x = np.linalg.solve(blocks, b.reshape(-1, n, 1))[..., 0].ravel()
    return x, combined


def _guess_block(m, size):
    """Smallest n whose n x n diagonal blocks hold every non-zero of m."""
    coo = sp.coo_matrix(m) if sp.issparse(m) else sp.coo_matrix(np.asarray(m))
    for n in range(1, 65):
        if size % n == 0 and np.all((coo.row // n) == (coo.col // n)):
            return n
    raise ValueError("matrix is not block diagonal")


def propagate_and_blend_prior(x_analysis, P_analysis, P_analysis_inverse, M_matrix, Q_matrix,
                              prior=None, state_propagator=None, date=None, reference_quirks: bool = True):
    """Propagator then prior blend (kf_tools.py:136-171).  ``reference_quirks``
    selects the reference's swapped blend (default, the reference API) or the
    Gaussian product; ``LinearKalman`` passes its ``EngineConfig.reference_quirks``
    so host and device blends agree."""
    if state_propagator is not None:
        x_forecast, P_forecast, P_forecast_inverse = state_propagator(
            x_analysis, P_analysis, P_analysis_inverse, M_matrix, Q_matrix)
    if prior is not None:
        prior_mean, prior_cov_inverse = prior.process_prior(date, inv_cov=True)
    if prior is not None and state_propagator is not None:
        x_combined, combined_cov_inv = blend_prior(prior_mean, prior_cov_inverse, x_forecast, P_forecast_inverse,
                                                   quirk=reference_quirks)
        return x_combined, None, combined_cov_inv
    elif prior is not None:
        return prior_mean, None, prior_cov_inverse
    elif state_propagator is not None:
        return x_forecast, P_forecast, P_forecast_inverse
    return None, None, None


# ------------------------------------------------------------- propagators
def propagate_standard_kalman(x_analysis, P_analysis, P_analysis_inverse, M_matrix, Q_matrix,
                              prior=None, state_propagator=None, date=None):
    """x_f = M x_a, P_f = P_a + Q (kf_tools.py:174-205)."""
    x_forecast = M_matrix.dot(x_analysis)
    P_forecast = P_analysis + Q_matrix
    return x_forecast, P_forecast, None


propagate_standard_kalman.device_spec = PropagatorSpec(PROP_STANDARD, output="covariance")


def propagate_information_filter_SLOW(x_analysis, P_analysis, P_analysis_inverse, M_matrix, Q_matrix,
                                      prior=None, state_propagator=None, date=None, n_params=None):
    """Exact information propagation P_f^-1 = (I + P_a^-1 Q)^-1 P_a^-1 (kf_tools.py:208-245),
    solved block by block."""
    x_forecast = _apply_M(M_matrix, x_analysis)
    n = n_params or _guess_block(P_analysis_inverse, len(x_forecast))
    Ai = sparse_to_blocks(P_analysis_inverse, n, check=False).astype(np.float64)
    q = _diag(Q_matrix).reshape(-1, n)
    lhs = np.eye(n)[None] + Ai * q[:, None, :]
    Pf = np.linalg.solve(lhs, Ai)
    return x_forecast, None, blocks_to_sparse(Pf, "csr")


propagate_information_filter_SLOW.device_spec = PropagatorSpec(PROP_INFO_EXACT)


def propagate_information_filter_approx_SLOW(x_analysis, P_analysis, P_analysis_inverse, M_matrix, Q_matrix,
                                             prior=None, state_propagator=None, date=None):
    """Diagonal approximation D = 1/(1 + diag(P^-1) diag(Q)) (kf_tools.py:247-289)."""
    x_forecast = _apply_M(M_matrix, x_analysis)
    d = _diag(P_analysis_inverse)
    D = 1. / (1. + d * _diag(Q_matrix))
    n = len(d)
    return x_forecast, None, sp.dia_matrix((d * D, 0), shape=(n, n)).tocsr()


propagate_information_filter_approx_SLOW.device_spec = PropagatorSpec(PROP_INFO_APPROX)

# the reference test-suite imports this name (tests/test_kf.py:16); its golden
# diagonal is the diagonal approximation's.
propagate_information_filter = propagate_information_filter_approx_SLOW


def make_partial_prior_propagator(prior_mean, prior_cov_inverse, propagated, name="partial_prior"):
    """Generalised ``propagate_information_filter_LAI``: every parameter is reset to
    the prior except the ``propagated`` indices, whose mean is carried by M and
    whose variance is inflated by Q: P_f^-1[k,k] = 1/(1/P_a^-1[k,k] + Q[k])."""
    prior_mean = np.asarray(prior_mean, dtype=np.float64)
    prior_cov_inverse = np.asarray(prior_cov_inverse, dtype=np.float64)
    n = prior_mean.size
    propagated = tuple(int(k) for k in np.atleast_1d(propagated))

    def propagator(x_analysis, P_analysis, P_analysis_inverse, M_matrix, Q_matrix,
                   prior=None, state_propagator=None, date=None):
        x_forecast = _apply_M(M_matrix, x_analysis)
        n_pixels = len(x_analysis) // n
        x0 = np.tile(prior_mean, n_pixels)
        blocks = np.broadcast_to(prior_cov_inverse, (n_pixels, n, n)).copy()
        dA = _diag(P_analysis_inverse)
        dQ = _diag(Q_matrix)
        for k in propagated:
            x0[k::n] = x_forecast[k::n]
            blocks[:, k, k] = 1.0 / ((1.0 / dA[k::n]) + dQ[k::n])
        return x0, None, blocks_to_sparse(blocks.astype(np.float32), "csr")

    propagator.__name__ = name
    propagator.device_spec = PropagatorSpec(PROP_PRIOR_PARTIAL, propagated=propagated, reset_mean=prior_mean,
                                            reset_cinv=prior_cov_inverse)
    return propagator


_tip_mean, _, _tip_cinv = tip_prior()
propagate_information_filter_LAI = make_partial_prior_propagator(_tip_mean, _tip_cinv, (6,),
                                                                 "propagate_information_filter_LAI")
propagate_information_filter_LAI.__doc__ = (
    "JRC-TIP LAI-only propagation (kf_tools.py:292-314): all parameters reset to the TIP prior "
    "except TLAI (index 6), whose precision is inflated by Q.")


def make_no_propagation(prior_mean, prior_cov_inverse, name="no_propagation"):
    prior_mean = np.asarray(prior_mean, dtype=np.float64)
    prior_cov_inverse = np.asarray(prior_cov_inverse, dtype=np.float64)
    n = prior_mean.size

    def propagator(x_analysis, P_analysis, P_analysis_inverse, M_matrix, Q_matrix,
                   prior=None, state_propagator=None, date=None):
        n_pixels = len(x_analysis) // n
        blocks = np.broadcast_to(prior_cov_inverse.astype(np.float32), (n_pixels, n, n))
        return np.tile(prior_mean, n_pixels), None, blocks_to_sparse(np.ascontiguousarray(blocks), "csr")

    propagator.__name__ = name
    propagator.device_spec = PropagatorSpec(PROP_PRIOR, reset_mean=prior_mean, reset_cinv=prior_cov_inverse)
    return propagator


no_propagation = make_no_propagation(_tip_mean, _tip_cinv)
no_propagation.__doc__ = "Reset to the tiled TIP prior, ignoring inputs (kf_tools.py:316-353)."


def identity_propagation(x_analysis, P_analysis, P_analysis_inverse, M_matrix, Q_matrix,
                         prior=None, state_propagator=None, date=None):
    """x_f = M x_a with the analysis precision carried unchanged."""
    return _apply_M(M_matrix, x_analysis), P_analysis, P_analysis_inverse


identity_propagation.device_spec = PropagatorSpec(PROP_IDENTITY)


# ---------------------------------------------------------------- smoother
def _mask_indices(mask, n):
    """Propagated parameter indices from a bit mask (bit j: parameter j) or a sequence of indices."""
    if isinstance(mask, (int, np.integer)):
        if mask < 0 or int(mask) >> n:
            raise ValueError(f"mask {int(mask):#x} has a bit at or above n={n}")
        return np.array([j for j in range(n) if (int(mask) >> j) & 1], dtype=np.int64)
    J = np.unique(np.asarray(list(mask), dtype=np.int64))
    if J.size and (J[0] < 0 or J[-1] >= n):
        raise ValueError(f"mask holds an index outside 0..{n - 1}")
    return J


def rts_smooth_blocks(x_a, blocks_a, x_next, P_next, mask, m, q, kind="precision"):
    """One backward step of the fixed-interval (Rauch-Tung-Striebel) smoother,
    per pixel, in float64 (no reference counterpart: the reference only filters).

    ``x_a`` [N, n] and ``blocks_a`` [N, n, n]: the filtered state of step t, the
    blocks holding P_a^-1 (``kind="precision"``) or P_a (``"covariance"``);
    ``x_next`` [N, n] and ``P_next`` [N, n, n]: the smoothed mean and covariance
    of step t + 1.  ``mask``: the parameters J the propagator carries from t to
    t + 1, as a bit mask or a sequence of indices; ``m`` [n]: the diagonal
    trajectory model; ``q`` [n] or [N, n]: the model error.  With M = diag(m)
    restricted to J::

        x_p = M x_a[J]                      P_p = M P_a[J, J] M + diag(q[J])
        G   = P_a[:, J] M P_p^-1
        x_s = x_a + G (x_next[J] - x_p)     P_s = P_a + G (P_next[J, J] - P_p) G^T

    Returns ``(x_s [N, n], P_s [N, n, n])``.  With an empty J nothing links the
    steps and the filtered moments are returned.  For the propagators whose
    forecast is exactly (x_p, P_p) -- standard, exact information filter,
    identity -- this is the classical RTS step and the chain of steps gives the
    batch posterior of the whole series."""
    if kind not in ("precision", "covariance"):
        raise ValueError("kind must be 'precision' or 'covariance'")
    x_a = np.asarray(x_a, dtype=np.float64)
    N, n = x_a.shape
    A = np.asarray(blocks_a, dtype=np.float64).reshape(N, n, n)
    P_a = np.linalg.inv(A) if kind == "precision" else A.copy()
    J = _mask_indices(mask, n)
    if J.size == 0:
        return x_a.copy(), P_a
    x_next = np.asarray(x_next, dtype=np.float64).reshape(N, n)
    P_next = np.asarray(P_next, dtype=np.float64).reshape(N, n, n)
    mJ = np.broadcast_to(np.asarray(m, dtype=np.float64), (n,))[J]
    qJ = np.broadcast_to(np.asarray(q, dtype=np.float64), (N, n))[:, J]
    x_p = x_a[:, J] * mJ
    P_p = P_a[:, J][:, :, J] * mJ[:, None] * mJ[None, :]
    P_p[:, np.arange(J.size), np.arange(J.size)] += qJ
    C = P_a[:, :, J] * mJ[None, None, :]                                  # P_a[:, J] M
    G = np.linalg.solve(P_p, C.transpose(0, 2, 1)).transpose(0, 2, 1)     # P_p symmetric
    x_s = x_a + np.einsum("pij,pj->pi", G, x_next[:, J] - x_p)
    D = P_next[:, J][:, :, J] - P_p
    P_s = P_a + np.einsum("pij,pjk,plk->pil", G, D, G)
    return x_s, 0.5 * (P_s + P_s.transpose(0, 2, 1))


# ------------------------------------------------------- Hessian correction
def hessian_correction_pixel(gp, x0, C_obs_inv, innovation, band, nparams):
    selecta = band_selecta(band)
    ddH = np.asarray(gp.hessian(np.atleast_2d(x0[selecta]))).squeeze()
    big = np.zeros((nparams, nparams))
    big[np.ix_(selecta, selecta)] = ddH
    return big * C_obs_inv * innovation


def hessian_correction(gp, x0, R_mat, innovation, mask, state_mask, band, nparams, state_map=None):
    """Second-order GN correction of the likelihood Hessian (kf_tools.py:37-60),
    vectorised over pixels.  Returns 0. if the emulator has no ``hessian``."""
    if not hasattr(gp, "hessian"):
        return 0.
    C_obs_inv = _diag(R_mat)[np.asarray(state_mask).ravel()]
    m = np.asarray(mask)[np.asarray(state_mask)].ravel().astype(bool)
    smap = band_selecta(band) if state_map is None else np.asarray(state_map)
    N = m.size
    x = np.asarray(x0).reshape(N, nparams)
    blocks = np.zeros((N, nparams, nparams))
    idx = np.nonzero(m)[0]
    if idx.size:
        ddH = np.asarray(gp.hessian(x[idx][:, smap]))
        scale = (C_obs_inv[idx] * np.asarray(innovation)[idx])[:, None, None]
        blocks[np.ix_(idx, smap, smap)] = ddH * scale
    return blocks_to_sparse(blocks, "csr")


def hessian_correction_multiband(gp, x0, R_mats, innovations, masks, state_mask, n_bands, nparams):
    """Sum of per-band corrections (kf_tools.py:63-72)."""
    gps = gp if isinstance(gp, (list, tuple)) else [gp] * n_bands
    return sum(hessian_correction(g, x0, R, inn, mk, state_mask, b, nparams)
               for g, R, inn, mk, b in zip(gps, R_mats, innovations, masks, range(n_bands)))


def _innovation_front(P, y, w, H0, h, kind, ok):
    """What ``innovation_blocks`` and ``evidence_blocks`` share: the inputs in
    float64, the covariance ``C`` (identity where the pixel is unscreenable),
    ``good`` [N], the raw ``z`` [nb, N] and the counted bands [nb, N]."""
    P = np.asarray(P, dtype=np.float64)
    y, w, H0 = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (y, w, H0))
    h = np.asarray(h, dtype=np.float64).reshape(y.shape + (P.shape[-1],))
    nb, N = y.shape
    good = np.isfinite(P).all(axis=(1, 2))
    safe = np.where(good[:, None, None], P, np.eye(P.shape[-1]))
    good &= np.all(np.linalg.eigvalsh(safe) > 0.0, axis=1)
    safe = np.where(good[:, None, None], P, np.eye(P.shape[-1]))
    C = np.linalg.inv(safe) if kind == "precision" else safe
    s = np.einsum("bpi,pij,bpj->bp", h, C, h)
    with np.errstate(all="ignore"):
        z = (y - H0) / np.sqrt(s + 1.0 / np.where(w > 0, w, 1.0))
    counted = (w > 0) & good[None, :] & np.isfinite(z) & np.isfinite(h).all(axis=2) & np.isfinite(H0)
    if ok is not None:
        counted &= np.asarray(ok, dtype=bool).reshape(nb, N)
    return y, w, H0, h, C, good, z, counted


def innovation_blocks(P, y, w, H0, h, kind="precision", gate=0.0, scope="group", groups=None, ok=None):
    """Float64 oracle of the innovation statistics and the chi-square gate
    (``ops.kernels.innovation``, csrc/kf_core.h ``pixel_innovation``) on host blocks.

    ``P`` [N, n, n]: the pixels' precision (``kind="precision"``) or covariance
    (``"covariance"``) blocks; ``y`` / ``w`` [nb, N]: the decoded observations
    and inverse variances (w <= 0: no observation); ``H0`` [nb, N] and ``h``
    [nb, N, n]: each band's operator value and Jacobian row at the state, in
    float64, so a caller can feed exact operator values; ``ok`` [nb, N] bool
    (optional): False where the operator is invalid.

    Returns ``(z, chi2, nobs, reject)``: z [nb, N] = (y - H0) / sqrt(h^T C h +
    1/w) with C the covariance, NaN where the band is not counted; chi2 [N] the
    sum of z^2 over the counted bands (not the joint Mahalanobis distance);
    nobs [N] the counted bands; reject [nb, N] bool -- with ``gate`` k > 0 band
    b where |z_b| > k (``scope="band"``), or every counted band of a group
    (``groups``: one id per band, None: one group) in which a band exceeds k
    (``scope="group"``).  A pixel whose block is not SPD or not finite is
    unscreenable: z and chi2 NaN, nobs 0, nothing rejected."""
    if kind not in ("precision", "covariance"):
        raise ValueError("kind must be 'precision' or 'covariance'")
    if scope not in ("band", "group"):
        raise ValueError("scope must be 'band' or 'group'")
    if not gate >= 0.0:
        raise ValueError("gate must be >= 0")
    y, w, H0, h, C, good, z, counted = _innovation_front(P, y, w, H0, h, kind, ok)
    nb, N = y.shape
    z = np.where(counted, z, np.nan)
    chi2 = np.where(good, np.sum(np.where(counted, z, 0.0) ** 2, axis=0), np.nan)
    nobs = counted.sum(axis=0).astype(np.int64)
    over = counted & (np.abs(np.where(counted, z, 0.0)) > gate) if gate > 0 else np.zeros_like(counted)
    if scope == "group" and over.any():
        g = np.zeros(nb, dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
        if g.shape != (nb,):
            raise ValueError("groups: one id per band")
        reject = np.zeros_like(counted)
        for gid in np.unique(g):
            sel = g == gid
            reject[sel] = over[sel].any(axis=0)[None, :]
        reject &= counted
    else:
        reject = over
    return z, chi2, nobs, reject


def evidence_blocks(P, y, w, H0, h, kind="precision", ok=None):
    """Float64 oracle of the joint innovation statistic and the Gaussian log
    evidence of one date (``ops.kernels.innovation`` ``d2`` / ``logdet``), on the
    inputs of ``innovation_blocks`` and with its counting rule.

    Per pixel, over the counted bands, S = H C H^T + diag(1 / w) with C the
    covariance and r = y - H0.  Returns ``(d2, logdet, nobs, loglik)``, each
    [N]: d2 = r^T S^-1 r (``np.linalg.solve``), logdet = log det S
    (``slogdet``), loglik = -(d2 + logdet + nobs log 2 pi) / 2: the textbook
    formula, free of the band order, not the kernel's band-by-band recursion.
    For nonlinear bands this is the linearised (extended-filter) evidence at the
    state H0 and h were evaluated at.  An unscreenable pixel gives NaN (nobs 0),
    a pixel with nothing counted zeros."""
    if kind not in ("precision", "covariance"):
        raise ValueError("kind must be 'precision' or 'covariance'")
    y, w, H0, h, C, good, _, counted = _innovation_front(P, y, w, H0, h, kind, ok)
    N = y.shape[1]
    d2 = np.zeros(N)
    logdet = np.zeros(N)
    for p in range(N):
        if not good[p]:
            d2[p] = logdet[p] = np.nan
            continue
        sel = counted[:, p]
        if not sel.any():
            continue
        Hp = h[sel, p]
        S = Hp @ C[p] @ Hp.T + np.diag(1.0 / w[sel, p])
        r = y[sel, p] - H0[sel, p]
        d2[p] = r @ np.linalg.solve(S, r)
        logdet[p] = np.linalg.slogdet(S)[1]
    nobs = counted.sum(axis=0).astype(np.int64)
    loglik = -0.5 * (d2 + logdet + nobs * np.log(2.0 * np.pi))
    return d2, logdet, nobs, loglik


def product_blocks(x, blocks, transforms, z, kind="precision", status=None, nobs=None, nrej=None):
    """Float64 oracle of ``ops.kernels.product`` (csrc/kf_core.h ``pixel_product``):
    the same definitions on the float32-rounded inputs and the float32 ``z``.

    ``x`` [N, n]; ``blocks`` [N, n, n], the precision (``kind="precision"``) or
    covariance blocks; ``transforms``: one ``ParameterTransform`` or None per
    parameter; ``status`` / ``nobs`` / ``nrej``: optional uint8 [N].  Returns
    ``(med, lower, upper, qa, clamped)``: the three [N, n_sel] product planes of
    the selected parameters (state order), the QA bytes [N] and ``clamped``
    [3, N, n_sel], the clamped arguments (of the median, of x - z sigma and of
    x + z sigma) the transforms were applied to."""
    from ..ops.kernels import ST_BAD_OP, ST_FALLBACK, ST_NO_OBS, ST_NONFINITE, ST_NONSPD, ST_OUT_OF_DOMAIN
    if kind not in ("precision", "covariance"):
        raise ValueError("kind must be 'precision' or 'covariance'")
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    A = np.asarray(blocks, dtype=np.float32).astype(np.float64)
    N, n = x.shape
    z = float(np.float32(z))
    transforms = list(transforms)
    if len(transforms) != n or A.shape != (N, n, n):
        raise ValueError("x [N, n], blocks [N, n, n] and one transform (or None) per parameter")
    var = np.full((N, n), np.nan)
    if kind == "covariance":
        var = np.diagonal(A, axis1=1, axis2=2).copy()
        block_ok = np.ones(N, bool)
    else:
        block_ok = np.isfinite(A).all(axis=(1, 2))
        for i in np.nonzero(block_ok)[0]:
            try:
                np.linalg.cholesky(A[i])
                var[i] = np.diagonal(np.linalg.inv(A[i]))
            except np.linalg.LinAlgError:
                block_ok[i] = False
        with np.errstate(invalid="ignore"):
            block_ok &= (np.isfinite(var) & (var > 0)).all(axis=1)
    with np.errstate(invalid="ignore"):
        var_ok = block_ok[:, None] & np.isfinite(var) & (var > 0)
    sel = [j for j, t in enumerate(transforms) if t is not None]
    med, lower, upper = (np.full((N, len(sel)), np.nan) for _ in range(3))
    clamped = np.full((3, N, len(sel)), np.nan)
    qa = np.zeros(N, dtype=np.uint8)
    if not sel and kind == "precision":
        qa[~block_ok] |= 16

    def clamp(u, lo, hi):                       # NaN stays NaN, as the kernel's
        with np.errstate(invalid="ignore"):
            return np.where(u < lo, lo, np.where(u > hi, hi, u))

    for s, j in enumerate(sel):
        t = transforms[j]
        _, _, lo, hi = t.f32()
        xj = x[:, j]
        have = var_ok[:, j] & np.isfinite(xj)
        sd = np.sqrt(np.where(have, var[:, j], 1.0))
        um, up = xj - z * sd, xj + z * sd
        c = clamped[:, :, s]
        c[0], c[1], c[2] = clamp(xj, lo, hi), clamp(um, lo, hi), clamp(up, lo, hi)
        f0, fm, fp = t.apply(c[0]), t.apply(c[1]), t.apply(c[2])
        med[:, s] = f0
        lower[:, s] = np.where(have, np.minimum(fm, fp), np.nan)
        upper[:, s] = np.where(have, np.maximum(fm, fp), np.nan)
        c[1:, ~have] = np.nan
        with np.errstate(invalid="ignore"):
            qa[~have] |= 16
            qa[(xj < lo) | (xj > hi)] |= 32
            qa[have & ((um < lo) | (um > hi) | (up < lo) | (up > hi))] |= 64
    st = np.zeros(N, np.uint8) if status is None else np.asarray(status, dtype=np.uint8)[:N]
    no = np.zeros(N, np.uint8) if nobs is None else np.asarray(nobs, dtype=np.uint8)[:N]
    nr = np.zeros(N, np.uint8) if nrej is None else np.asarray(nrej, dtype=np.uint8)[:N]
    qa[((st & ST_NO_OBS) != 0) | ((no > 0) & (nr >= no))] |= 1
    qa[(st & (ST_FALLBACK | ST_NONSPD | ST_NONFINITE | ST_BAD_OP)) != 0] |= 2
    qa[(st & ST_OUT_OF_DOMAIN) != 0] |= 4
    qa[nr > 0] |= 8
    return med, lower, upper, qa, clamped
