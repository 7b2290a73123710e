"""Hessian tables of the matrix-core K6 (models/gp.py:mfma_hessian_tables, the
operand layout of csrc/kf_gp_mfma.h gp_hessian_sums) on the CPU, and the host
function that chooses the kernel (csrc/kf_plan.h hessian_plan).

The bound of the float64 comparison is derived, not tuned.  A term of a sum is
A_f,i m_i with m_i = 2^E_i, E_i = L'_i + c + sum_d B_id xi_d.  Split-f16 keeps
22 bits of an operand, so every product loses at most 2^-22 of its magnitude
per operand: A (one split) and m (hi truncated, lo rounded: 2^-21) give
3 x 2^-22; each exponent product B_d xi_d has two splits and the dropped
lo x lo part, 3 x 2^-22 |B_d xi_d|, which m carries as ln2 times that.  The
float32 records the tables are built from add 2^-24 on L' and each B_d in the
exponent and 2 x 2^-24 on a field B_u B_v.  A term's relative error is
therefore at most
  2^-22 (3.5 + ln2 (3.25 sum_d |B_d xi_d| + 0.25 |L'|)),
and the bound of an entry is that times the term scale sum |alpha k| of the
entry's assembly, lambda_u lambda_v (|xi_u| + |t_u|) (|xi_v| + |t_v|) (plus
lambda_u on the diagonal)."""
import numpy as np
import pytest

from kafka_inferenceengine_amd.models import gp
from kafka_inferenceengine_amd.models.operators import OP_SAR
from kafka_inferenceengine_amd.ops import kernels as K


def _emulator(D, n_train, seed=0):
    rng = np.random.default_rng([seed, D, n_train])
    v = rng.normal(size=D)
    return gp.GaussianProcessEmulator.synthetic(lambda X: 0.4 + 0.2 * np.sin(X @ v), np.zeros(D), np.ones(D),
                                                n_train=n_train, seed=seed + D)


@pytest.mark.parametrize("n_train", [24, 40, 70])
@pytest.mark.parametrize("D", [2, 4, 10])
def test_fragment_model_matches_float64_hessian(D, n_train):
    em = _emulator(D, n_train)
    tab, nch, scale, fs = gp.mfma_hessian_tables(em.records(), em.n_pos_pairs, em.lam)
    assert nch == -(-n_train // 32)
    assert tab.shape == (nch, gp.hess_frags_per_chunk(D), 8) and fs.shape == (gp.hess_fields(D),)
    assert np.all(np.log2(fs) == np.round(np.log2(fs)))
    X = np.random.default_rng(D).uniform(0.05, 0.95, (200, D))
    xi = X - em.center()[None]
    c = -0.5 * gp.LOG2E * (em.lam[None] * xi * xi).sum(1)
    S0, H = gp.hessian_from_sums(gp.mfma_hessian_emulate(tab, nch, scale, fs, D, xi, c), em.lam, xi)
    t = em.inputs - em.center()[None]                                   # [T, D]
    ak = np.abs(em.alpha[None] * em._kernel(X)[2])                      # [n, T]
    L = np.log2(em.signal * np.abs(em.alpha)) - 0.5 * gp.LOG2E * (t * t * em.lam).sum(1)
    Bx = np.abs((gp.LOG2E * em.lam * t)[None] * xi[:, None, :]).sum(2)  # [n, T]
    W = ak * 2.0 ** -22 * (3.5 + np.log(2.0) * (3.25 * Bx + 0.25 * np.abs(L)[None]))
    g = em.lam * (np.abs(xi)[:, None, :] + np.abs(t)[None])             # [n, T, D]
    bound = np.einsum("nt,ntu,ntv->nuv", W, g, g) + W.sum(1)[:, None, None] * np.diag(em.lam)[None]
    assert np.all(np.abs(H - em.hessian(X)) <= bound)
    assert np.all(np.abs(em.mean + S0 - em.predict(X)[0]) <= W.sum(1))


def _records(B, L=None):
    """Records of one positive pair per two points with the given B [T, D]."""
    B = np.asarray(B, dtype=np.float64)
    pts = np.concatenate([np.zeros((B.shape[0], 1)) if L is None else np.asarray(L)[:, None], B], 1)
    return pts.reshape(-1, 2, pts.shape[1]).transpose(0, 2, 1).astype(np.float32)


def test_field_scales_keep_products_in_f16_range():
    """B_u B_v = 9e4 is beyond f16 (65504) and 1e-9 below it; both build, scaled."""
    B = np.array([[300.0, 300.0], [1e-5, 1e-4], [3.0, -2.0], [0.5, 0.25]])
    r = gp.mfma_hessian_tables(_records(B), 2, np.array([1e4, 1e4]))
    assert r is not None
    tab, nch, _, fs = r
    assert np.isfinite(tab.astype(np.float64)).all() and fs[3] < 1.0
    S = gp.mfma_hessian_emulate(tab, nch, r[2], fs, 2, np.zeros((1, 2)), np.zeros(1))
    want = [4.0] + list(B.sum(0)) + [(B[:, u] * B[:, v]).sum() for u, v in ((0, 0), (0, 1), (1, 1))]
    assert np.allclose(S[0], want, rtol=2.0 ** -20, atol=0)


def test_band_that_cannot_fit_has_no_table():
    assert gp.mfma_hessian_tables(_records(np.array([[1e5, 0.0], [1.0, 1.0]])), 1, np.ones(2)) is None


def _desc(op=K.OP_GP, d=4):
    b = K.ext().BandDesc()
    b.op, b.d = op, d
    return b


@pytest.mark.parametrize("np_, descs, tabs, device, want", [
    (7, [(K.OP_GP, 4)] * 2, [1, 1], True, "hessian_mfma_kernel<7, 4>"),
    (10, [(K.OP_GP, 10)] * 3, [1, 1, 1], True, "hessian_mfma_kernel<10, 10>"),
    (7, [(K.OP_GP, 4), (OP_SAR, 2), (K.OP_GP, 4)], [1, 0, 1], True, "hessian_mfma_kernel<7, 4>"),   # a SAR band beside GPs
    (4, [(K.OP_GP, 4)] * 2, [1, 1], True, "pixel_kernel<4, kf::OpHessian>"),
    (7, [(K.OP_GP, 4)] * 2, [1, 0], True, "pixel_kernel<7, kf::OpHessian>"),                   # a missing table
    (7, [(K.OP_GP, 4)] * 2, [1, 1], False, "pixel_kernel<7, kf::OpHessian>"),                  # the host
])
def test_hessian_plan_rows(np_, descs, tabs, device, want):
    bands = [_desc(op, d) for op, d in descs]
    plan = K.ext().hessian_plan(np_, bands, [0x1000 * t for t in tabs], [0x2000 * t for t in tabs],
                                [2 * t for t in tabs], [1.0] * len(tabs), device)
    assert plan["name"] == want
    assert "hessian_mfma_kernel<7, 4>" in K.ext().hessian_table()
