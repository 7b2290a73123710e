"""The auxiliary kernels -- K7 (nearest LUT row), propagate, invert, the
standalone operator evaluation, the K2 split path (gp_operator), the K6
Hessian correction, unpack and gather -- at every compiled state size, against
float64 NumPy models of the same operation (never the kernels' own source),
with a leading dimension larger than N, a sentinel in every padding column and
N below, at and above one wave and across two workgroups.

Each test runs on the CPU (the host runner built from the same per-pixel
source) and, marked ``gpu``, on the MI355X.  Problem builders and the float64
models live in ``kernel_cases.py``.

Tolerances are the project's existing ones: ``x_err`` / ``a_err`` of
test_oracles.py with x 1e-5 (1e-4 with the blend) and P 1e-5 (1e-4 for the
exact information filter); invert ``rtol=1e-4, atol=1e-6``; the Hessian 2e-3
of the largest entry of the correction; unpack's mean exact and its
uncertainty ``rtol=1e-6``; gather and the K7 index exact; the operators those of
tests/test_kernels.py:191-225 (precomputed rows exact, linear ``atol=1e-5``, SAR
``rtol=2e-5`` and for the gradient ``rtol=2e-4, atol=1e-7``, GP ``atol=5e-6``
and for the gradient ``5e-5``).

Worst measured errors over all modes, blends and N (the tests print them).
propagate: x without / with the blend, P of every mode but the exact filter /
of the exact filter.  invert: the largest |err| / (atol + rtol |ref|), 1 being
the bound.  hessian: of the largest entry.  unpack: relative, uncertainty.
operator_eval and gp_operator: the largest |err| / (atol + rtol |ref|) of the
value / of the gradient, 1 being the bound; the same figures, digit for digit,
with the kernels as they were before pixel_kernel replaced them.

    kernel           n   host runner                       MI355X
    ---------------  --  --------------------------------  --------------------------------
    propagate        1   5.6e-8 1.3e-6 / 1.1e-7 2.6e-7     5.6e-8 9.1e-7 / 1.1e-7 2.1e-7
    propagate        2   5.5e-8 9.2e-7 / 1.2e-7 2.9e-7     5.5e-8 8.7e-7 / 1.2e-7 3.0e-7
    propagate        3   5.6e-8 2.3e-6 / 1.2e-7 2.6e-7     5.6e-8 2.7e-6 / 1.1e-7 1.8e-7
    propagate        4   5.4e-8 2.3e-6 / 1.1e-7 3.1e-7     5.4e-8 2.0e-6 / 1.2e-7 2.6e-7
    propagate        7   5.5e-8 3.5e-6 / 1.2e-7 3.8e-7     5.5e-8 3.3e-6 / 1.2e-7 4.0e-7
    propagate        10  5.7e-8 7.0e-6 / 1.0e-7 4.1e-7     5.7e-8 5.9e-6 / 1.2e-7 3.9e-7
    invert           1   1.6e-3                            1.6e-3
    invert           2   2.3e-3                            1.9e-3
    invert           3   2.4e-3                            2.5e-3
    invert           4   3.3e-3                            2.5e-3
    invert           7   3.4e-3                            3.1e-3
    invert           10  4.7e-3                            4.7e-3
    hessian tip      7   1.9e-5                            2.0e-5
    hessian prosail  10  4.8e-6                            4.8e-6
    hessian d = n    2   2.2e-5                            2.4e-5
    hessian d = n    3   1.5e-5                            1.5e-5
    hessian d = n    4   1.1e-5                            1.1e-5
    unpack           1   8.2e-8                            7.5e-8
    unpack           2   8.2e-8                            7.7e-8
    unpack           3   8.5e-8                            8.7e-8
    unpack           4   8.4e-8                            9.3e-8
    unpack           7   8.5e-8                            8.2e-8
    unpack           10  8.9e-8                            8.9e-8
    operator linear  1   1.5e-3 / 0                        1.5e-3 / 0
    operator linear  2   2.5e-3 / 0                        2.5e-3 / 0
    operator linear  3   3.0e-3 / 0                        3.0e-3 / 0
    operator linear  4   3.7e-3 / 0                        3.7e-3 / 0
    operator linear  7   7.2e-3 / 0                        7.2e-3 / 0
    operator linear  10  5.6e-3 / 0                        5.6e-3 / 0
    operator sar     2   1.8e-2 / 7.6e-3                   1.8e-2 / 1.0e-2
    operator sar     3   2.1e-2 / 1.1e-2                   1.8e-2 / 1.1e-2
    operator sar     4   1.8e-2 / 1.5e-2                   1.8e-2 / 1.5e-2
    operator sar     7   1.8e-2 / 8.5e-3                   1.9e-2 / 8.5e-3
    operator sar     10  2.0e-2 / 2.2e-2                   1.8e-2 / 2.2e-2
    operator gp      1   1.3e-1 / 4.0e-2                   1.3e-1 / 3.9e-2
    operator gp      2   1.9e-1 / 4.2e-2                   2.0e-1 / 3.9e-2
    operator gp      3   1.3e-1 / 3.0e-2                   1.3e-1 / 2.9e-2
    operator gp      4   5.4e-2 / 9.2e-3                   5.4e-2 / 9.9e-3
    operator gp      7   2.0e-2 / 3.5e-3                   2.0e-2 / 3.5e-3
    operator gp      10  1.4e-2 / 2.0e-3                   1.4e-2 / 2.1e-3
    gp_operator 2,2  2   2.6e-1 / 4.1e-2                   2.7e-1 / 4.1e-2
    gp_operator 3,3  3   1.3e-1 / 4.2e-2                   1.3e-1 / 4.2e-2
    gp_operator 4,4  4   4.6e-2 / 1.1e-2                   4.6e-2 / 1.1e-2
    gp_operator 7,7  7   1.9e-2 / 3.1e-3                   1.9e-2 / 3.1e-3
    gp_operator 10,10 10 1.4e-2 / 2.4e-3                   1.4e-2 / 2.4e-3
    gp_operator 7,4  7   1.5e-1 / 3.2e-2                   1.5e-1 / 3.2e-2

The device's hardware reciprocal and reciprocal square root (kf_core.h kf_rcp,
kf_rsqrt) leave it inside every project tolerance at every state size; no
bound had to be derived from them.

K7: the device index equals the host runner's at every (M, D, N), and both
equal the float64 argmin on every pixel of every size (agreement 1.0, no
chosen row farther than the float64 minimum).  gather: exact.
"""
import numpy as np
import pytest
import torch

from kafka_inferenceengine_amd.ops import kernels as K
from kafka_inferenceengine_amd.utils.blocks import ntri, pack_blocks, unpack_blocks

import kernel_cases as C

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
MODES = (0, 1, 2, 3, 4, 5)


@pytest.fixture(params=DEVICES)
def dev(request):
    if request.param == "cuda":
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        return torch.device("cuda", 0)
    return torch.device("cpu")


def x_err(x, xr):
    return float(np.max(np.abs(x - xr) / (np.abs(xr) + 0.05)))


def a_err(A, Ar):
    d = np.sqrt(np.einsum("nii->ni", Ar))
    return float(np.max(np.abs(A - Ar) / (d[:, :, None] * d[:, None, :])))


def pad_untouched(t, N, fill=C.SENTINEL):
    """Columns N.. of a [rows, ld] (or [ld]) tensor still hold the sentinel, bit for bit."""
    tail = t[..., N:]
    return torch.equal(tail, torch.full_like(tail, fill))


# ------------------------------------------------------------------ K7
@pytest.mark.parametrize("M,D", C.LUT_SIZES)
def test_lut_nearest_vs_host_runner_and_float64(dev, M, D):
    """K7 at the reference's LUT sizes (4096 x 4 floats fill 64 KiB, 5000 x 10
    is the default LUT over a PROSAIL state).  The device index is the host
    runner's exactly (same fmaf order in float32); the float64 squared distance
    of the chosen row is within (1 + 1e-5) of the float64 minimum on every
    pixel and the index is the float64 argmin on at least 99.9 % of them."""
    c = C.lut_case(M, D)
    for N in C.LUT_N:
        got = C.lut_launch(c["lut"], c["pts"], N, dev)
        host = got if dev.type == "cpu" else C.lut_launch(c["lut"], c["pts"], N, "cpu")
        assert torch.equal(got, host), (M, D, N, int((got != host).sum()))
        assert bool((got[N:] == -7).all()), "wrote past N"
        idx = got[:N].numpy()
        assert idx.min() >= 0 and idx.max() < M
        d = C.lut_dist(c["lut"], c["pts"][:N], idx)
        same = float((idx == c["near"][:N]).mean())
        worst = float(np.max(d / np.maximum(c["dmin"][:N], 1e-300)))
        print(f"K7 M={M} D={D} N={N} on {dev}: argmin agreement {same:.5f}, worst d/dmin - 1 {worst - 1:.1e}")
        assert np.all(d <= (1.0 + 1e-5) * c["dmin"][:N]), worst
        assert same >= 0.999, same


def test_lut_nearest_ties_take_the_lowest_index(dev):
    """A duplicated LUT row (row 4000 == row 3, in different LDS chunks of the
    device kernel) is reported as the lower index; a pixel equal to a LUT row
    gets that row."""
    c = C.lut_case(5000, 4)
    lut = c["lut"].copy()
    lut[4000] = lut[3]
    rows = np.array([3, 4000, 0, 4999, 3071, 3072, 3073, 17, 4000, 3])
    pts = np.concatenate([lut[rows], c["pts"][:65]])
    # points near the duplicated row: nearer to it than to any other row
    pts[10:14] = lut[3] + 1e-4 * np.array([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, 1, 0], [0, 0, 0, -1]])
    pts = C.f32(pts)
    got = C.lut_launch(lut, pts, len(pts), dev)[:len(pts)].numpy()
    assert list(got[:10]) == [3, 3, 0, 4999, 3071, 3072, 3073, 17, 3, 3]
    others = np.delete(np.arange(5000), [3, 4000])
    for i in range(10, 14):
        assert C.lut_dist(lut, pts[i:i + 1], [3])[0] < C.lut_dist(lut[others], pts[i][None], np.arange(4998)).min()
    assert list(got[10:14]) == [3, 3, 3, 3]
    assert not np.any(got == 4000)


# ------------------------------------------------------------------ propagate
@pytest.mark.parametrize("blend", C.PROP_BLENDS)
@pytest.mark.parametrize("n", C.AUX_NP)
def test_propagate_every_state_size_vs_float64(dev, n, blend):
    """Modes 0-5 with per-pixel trajectory uncertainty (``q_pix``) and, with
    the blend, per-pixel prior mean and precision; the constant fields they
    replace are set to values that would be visibly wrong."""
    worst_x = worst_p = 0.0
    for mode in MODES:
        N, pad = C.aux_shape(C.AUX_NP.index(n) + mode + C.PROP_BLENDS.index(blend))
        c = C.propagate_case(n, N, mode, blend)
        xf, pf, _ = C.propagate_launch(c, dev, pad)
        assert pad_untouched(xf, N) and pad_untouched(pf, N), (mode, N, pad)
        ex = x_err(xf[:, :N].numpy().T.astype(np.float64), c["xf"])
        ep = a_err(unpack_blocks(pf[:, :N].numpy().astype(np.float64), n), c["P"])
        worst_x, worst_p = max(worst_x, ex), max(worst_p, ep)
        print(f"propagate n={n} mode={mode} blend={blend} N={N} ld={N + pad} on {dev}: x {ex:.2e} P {ep:.2e}")
        assert ex < (1e-5 if blend == "off" else 1e-4), (mode, N, ex)
        assert ep < (1e-4 if mode == 3 else 1e-5), (mode, N, ep)
    print(f"propagate n={n} blend={blend} on {dev}: worst x {worst_x:.2e} P {worst_p:.2e}")


@pytest.mark.parametrize("case", ["exact", "blend"])
@pytest.mark.parametrize("n", C.AUX_NP)
def test_propagate_flags_exactly_the_non_spd_pixels(dev, n, case):
    """Chosen pixels get p_a = -I: the exact information filter (the Cholesky
    factor of p_a) and the blend (that of P + C^-1) set ST_NONSPD on exactly
    those pixels; every other pixel's output equals the clean twin's bit for bit."""
    N, pad = C.aux_shape(C.AUX_NP.index(n) + (case == "blend"))
    mode, blend = (3, "off") if case == "exact" else (5, "on")
    c = C.propagate_case(n, N, mode, blend, seed=1)
    bad = np.zeros(N, bool)
    bad[[N - 1, N // 2, (N * 7) // 8]] = True
    A, Ci = c["A"].copy(), c["Ci"].copy()
    A[bad] = -np.eye(n)
    if case == "blend":
        # a prior precision below I: P + C^-1 stays indefinite on the bad pixels
        Ci = 0.1 * Ci / np.linalg.eigvalsh(Ci).max()
        assert np.linalg.eigvalsh(A + Ci)[bad].min() < 0 < np.linalg.eigvalsh(c["A"] + Ci).min()
    xa, pa, sa = C.propagate_launch(c, dev, pad, A=A, Ci=Ci, status=True)
    xb, pb, sb = C.propagate_launch(c, dev, pad, Ci=Ci, status=True)
    assert np.array_equal(sa[:N].numpy() & K.ST_NONSPD != 0, bad)
    assert np.array_equal(sa[:N].numpy() & ~np.uint8(K.ST_NONSPD), np.zeros(N, np.uint8))
    assert not sb[:N].any()
    assert bool((sa[N:] == 0xA5).all()) and bool((sb[N:] == 0xA5).all())
    good = torch.from_numpy(~bad)
    assert torch.equal(xa[:, :N][:, good], xb[:, :N][:, good]) and torch.equal(pa[:, :N][:, good], pb[:, :N][:, good])
    assert pad_untouched(xa, N) and pad_untouched(pa, N)


# ------------------------------------------------------------------ invert
@pytest.mark.parametrize("n", C.AUX_NP)
def test_invert_every_state_size_vs_float64(dev, n):
    """Packed SPD inverse against numpy.linalg.inv in float64, and the status
    bit on exactly the pixels whose block is not positive definite."""
    for i in range(len(C.AUX_N)):
        N, pad = C.aux_shape(C.AUX_NP.index(n) + i)
        ld = N + pad
        c = C.invert_case(n, N)
        dst = C.sentinel(ntri(n), ld, dev)
        K.invert(n, C.padded(pack_blocks(c["B"]), ld, dev), dst, N=N)
        dst = dst.cpu()
        got = unpack_blocks(dst[:, :N].numpy().astype(np.float64), n)
        err = float(np.max(np.abs(got - c["inv"]) / (1e-6 + 1e-4 * np.abs(c["inv"]))))
        print(f"invert n={n} N={N} ld={ld} on {dev}: |err| / (atol + rtol |ref|) {err:.2e}")
        assert np.allclose(got, c["inv"], rtol=1e-4, atol=1e-6), (N, err)
        assert pad_untouched(dst, N)
        # the same blocks with some made indefinite, and a status vector
        st = torch.zeros(ld, dtype=torch.uint8, device=dev)
        st[N:] = 0xA5
        dst2 = C.sentinel(ntri(n), ld, dev)
        K.invert(n, C.padded(pack_blocks(c["B_bad"]), ld, dev), dst2, N=N, status=st)
        st, dst2 = st.cpu(), dst2.cpu()
        assert np.array_equal(st[:N].numpy(), np.where(c["bad"], K.ST_NONSPD, 0).astype(np.uint8)), N
        assert bool((st[N:] == 0xA5).all()) and pad_untouched(dst2, N)
        good = torch.from_numpy(~c["bad"])
        assert torch.equal(dst2[:, :N][:, good], dst[:, :N][:, good])


# ------------------------------------------------------------------ operator_eval
OPERATOR_BANDS = (("precomp", K.OBS_F32), ("precomp", K.OBS_DN16), ("linear", K.OBS_F32), ("sar", K.OBS_F32),
                  ("gp", K.OBS_F32))
# (value, gradient) bounds as allclose keywords, tests/test_kernels.py:191-225; precomputed rows are copied
OPERATOR_TOL = {"linear": (dict(rtol=0, atol=1e-5), dict(rtol=0, atol=1e-5)),
                "sar": (dict(rtol=2e-5, atol=1e-8), dict(rtol=2e-4, atol=1e-7)),
                "gp": (dict(rtol=0, atol=5e-6), dict(rtol=0, atol=5e-5))}
# lanes of the first block whose precomputed rows carry a planted NaN / Inf (kernel_cases.nongp_case)
PLANTED = ((45, 47, 48), (46, 47))


def bound_use(got, ref, rtol, atol):
    """The largest |got - ref| / (atol + rtol |ref|): 1 is allclose's bound."""
    return float(np.max(np.abs(got - ref) / (atol + rtol * np.abs(ref)))) if got.size else 0.0


@pytest.mark.parametrize("n", C.AUX_NP)
def test_operator_eval_every_state_size(dev, n):
    """One band at a time over precomputed (two bands, NaN / Inf planted in
    their rows), linear, SAR (n >= 2) and GP (small_gp(n)) operators: H0, the
    Jacobian rows and ``ok`` against the case's float64 ``evals``; ``ok`` is 0 on
    exactly the planted pixels; a launch without ``h`` and ``ok`` gives the same
    H0 bit for bit; every padding column keeps its sentinel."""
    bands = tuple(b for b in OPERATOR_BANDS if n >= 2 or b[0] != "sar")
    worst = {}
    for i in range(len(C.AUX_N)):
        N, pad = C.aux_shape(C.AUX_NP.index(n) + i)
        ld = N + pad
        c = C.nongp_case(n, N, bands)
        tab, _ = C.nongp_table(c, dev, pad)
        x = C.padded(c["x0"].T, ld, dev, fill=-777.0)
        for b, (op, _) in enumerate(bands):
            H, hr = c["evals"][b][:2]
            h0, h = C.sentinel(1, ld, dev)[0], C.sentinel(n, ld + 7, dev)
            ok = torch.full((ld,), 0xA5, dtype=torch.uint8, device=dev)
            K.operator_eval(n, tab, b, x, h0, h, ok, N=N)
            h0b = C.sentinel(1, ld, dev)[0]
            K.operator_eval(n, tab, b, x, h0b, N=N)
            assert torch.equal(h0b.view(torch.int32), h0.view(torch.int32)), (op, N)
            h0, h, ok = h0.cpu(), h.cpu(), ok.cpu()
            assert pad_untouched(h0, N) and pad_untouched(h, N) and bool((ok[N:] == 0xA5).all()), (op, N, pad)
            bad = ~(np.isfinite(H) & np.isfinite(hr).all(1))
            assert np.array_equal(ok[:N].numpy(), np.where(bad, 0, 1).astype(np.uint8)), (op, N)
            want = [p for p in PLANTED[b] if p < N] if op == "precomp" else []
            assert np.flatnonzero(bad).tolist() == want, (op, N)
            g0, g = h0[:N].numpy(), h[:, :N].numpy().T
            if op == "precomp":
                assert np.array_equal(g0, H.astype(np.float32), equal_nan=True), (op, N)
                assert np.array_equal(g, hr.astype(np.float32), equal_nan=True), (op, N)
                continue
            tv, tg = OPERATOR_TOL[op]
            e = (bound_use(g0.astype(np.float64), H, **tv), bound_use(g.astype(np.float64), hr, **tg))
            worst[op] = tuple(max(a, b_) for a, b_ in zip(worst.get(op, (0.0, 0.0)), e))
            assert np.allclose(g0, H, **tv), (op, N, e)
            assert np.allclose(g, hr, **tg), (op, N, e)
    print(f"operator_eval n={n} on {dev}: worst error / bound (value, gradient) " +
          ", ".join(f"{op} {v:.2e} {g:.2e}" for op, (v, g) in worst.items()))


# ------------------------------------------------------------------ gp_operator
GP_OPERATOR_SHAPES = ((2, 2), (3, 3), (4, 4), (7, 7), (10, 10), (7, 4))
_TIP_CASES: dict = {}


def gp_operator_case(n, d, N):
    """-> (x0 [N, n] float32-valued, evals [(H0, h, y, w)] in float64, table builder):
    two small_gp(n) bands in two encodings, or the two JRC-TIP bands (d = 4)."""
    if d == n:
        c = C.nongp_case(n, N, (("gp", K.OBS_F32), ("gp", K.OBS_DN16)))
        return c["x0"], c["evals"], lambda dev, pad: C.nongp_table(c, dev, pad)[0]
    if N not in _TIP_CASES:
        prob = C.tip_problem(N=N, seed=11, dn16=True, mask_frac=0.3)
        x = C.f32(prob["x"])
        _TIP_CASES[N] = (prob, x, C.oracle_bands(prob, x))
    prob, x, evals = _TIP_CASES[N]
    return x, evals, lambda dev, pad: C.table(prob, dev)


@pytest.mark.parametrize("n,d", GP_OPERATOR_SHAPES)
def test_gp_operator_shapes_vs_float64(dev, n, d):
    """K2 split path, two bands per launch, each masked on a subset of the
    pixels: d = n with small_gp(n) bands and (7, 4) with the two JRC-TIP bands.
    Observed pixels against the float64 emulator (value 5e-6, gradient 5e-5),
    masked pixels exact zeros in h0 and all n rows, padding untouched.  (10, 4)
    keeps the coverage it has through the engine's split-path test
    (tests/test_engine.py test_split_gp_operator_path_equals_fused)."""
    worst = [0.0, 0.0]
    for i in range(len(C.AUX_N)):
        N, pad = C.aux_shape(GP_OPERATOR_SHAPES.index((n, d)) + i)
        ld, ldh = N + pad, N + pad + 3
        x0, evals, table = gp_operator_case(n, d, N)
        tab = table(dev, pad)
        h0, h = C.sentinel(2, ldh, dev), C.sentinel(2 * n, ldh, dev)
        K.gp_operator(n, tab, C.padded(x0.T, ld, dev, fill=-777.0), h0, h, N=N, d=d)
        h0, h = h0.cpu(), h.cpu()
        assert pad_untouched(h0, N) and pad_untouched(h, N), (N, pad)
        n_masked = 0
        for b, (H, hr, _, w) in enumerate(evals):
            on = w > 0
            n_masked += int((~on).sum())
            g0, g = h0[b, :N].numpy(), h[b * n:(b + 1) * n, :N].numpy().T
            assert not g0[~on].any() and not g[~on].any(), (b, N)
            assert not np.signbit(g0[~on]).any() and not np.signbit(g[~on]).any(), (b, N)
            e = (bound_use(g0[on].astype(np.float64), H[on], 0, 5e-6), bound_use(g[on].astype(np.float64), hr[on], 0, 5e-5))
            worst = [max(a, b_) for a, b_ in zip(worst, e)]
            assert np.allclose(g0[on], H[on], rtol=0, atol=5e-6), (b, N, e)
            assert np.allclose(g[on], hr[on], rtol=0, atol=5e-5), (b, N, e)
        assert N < 63 or n_masked > 0, "the case must mask some pixels"
    print(f"gp_operator n={n} d={d} on {dev}: worst error / bound value {worst[0]:.2e} gradient {worst[1]:.2e}")


# ------------------------------------------------------------------ hessian
@pytest.mark.parametrize("layout", C.HESSIAN_LAYOUTS)
def test_hessian_layouts_vs_float64(dev, layout):
    """K6 for the JRC-TIP layout (d = 4 in n = 7), three full-state PROSAIL-like
    bands (d = n = 10) and d = n in {2, 3, 4}, subtracted in place from a
    non-zero packed matrix; masked pixels keep theirs bit for bit."""
    for i in range(len(C.AUX_N)):
        N, pad = C.aux_shape(C.HESSIAN_LAYOUTS.index(layout) + i)
        c = C.hessian_case(layout, N)
        n = c["n"]
        a = C.hessian_launch(c, dev, pad)
        assert pad_untouched(a, N), (N, pad)
        got = unpack_blocks(a[:, :N].numpy().astype(np.float64), n)
        scale = np.abs(c["corr"]).max()
        err = float(np.max(np.abs(got - c["ref"])) / (scale + 1e-9))
        print(f"hessian {layout} n={n} N={N} ld={N + pad} on {dev}: {err:.2e} of the largest entry ({scale:.2e})")
        assert scale > 1e-3, "the correction must be visible next to a0"
        assert err < 2e-3, (N, err)
        m = c["masked"]
        assert np.array_equal(a[:, :N].numpy()[:, m], c["a0"].astype(np.float32)[:, m])


# ------------------------------------------------------------------ unpack
@pytest.mark.parametrize("outs", ["mean", "unc", "both"])
@pytest.mark.parametrize("mapped", [True, False])
@pytest.mark.parametrize("n", C.AUX_NP)
def test_unpack_every_state_size(dev, n, mapped, outs):
    """Mean (exact) and 1/sqrt(diag) (rtol 1e-6) through an index map or the
    identity into a raster larger than N; cells no pixel names keep the sentinel."""
    i = C.AUX_NP.index(n) + 2 * mapped + ("mean", "unc", "both").index(outs)
    N, pad = C.aux_shape(i)
    ld = N + pad
    c = C.unpack_case(n, N)
    plane = c["plane"] if mapped else N + 9
    cells = c["idx"] if mapped else np.arange(N)
    mean = C.sentinel(n, plane, dev) if outs != "unc" else None
    unc = C.sentinel(n, plane, dev) if outs != "mean" else None
    # the operands' padding holds -777 and the map's the raster's last cell (which no pixel
    # names): a pixel past N would leave a value that is not the sentinel in an unnamed cell
    idx = torch.from_numpy(np.concatenate([c["idx"], np.full(pad, plane - 1)])).to(dev) if mapped else None
    K.unpack(n, C.padded(c["x"].T, ld, dev, fill=-777.0),
             C.padded(pack_blocks(c["A"]), ld, dev, fill=-777.0) if unc is not None else None, mean, unc, idx=idx, N=N)
    rest = np.ones(plane, bool)
    rest[cells] = False
    for t in (mean, unc):
        if t is not None:
            assert bool((t.cpu()[:, torch.from_numpy(rest)] == C.SENTINEL).all())
    if mean is not None:
        assert np.array_equal(mean.cpu().numpy()[:, cells], c["x"].T.astype(np.float32))
    if unc is not None:
        ref = 1.0 / np.sqrt(np.einsum("nii->ni", c["A"])).T
        got = unc.cpu().numpy()[:, cells].astype(np.float64)
        print(f"unpack n={n} N={N} ld={ld} on {dev}: unc {float(np.max(np.abs(got / ref - 1))):.2e}")
        assert np.allclose(got, ref, rtol=1e-6)


# ------------------------------------------------------------------ gather
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16, torch.float32])
def test_gather_types_rows_strides_and_missing_sources(dev, dtype, rows):
    """out[r, p] = src[r, idx[p]] from a row-strided source view, about a tenth
    of the indices -1 (-> 0), into a destination wider than the index vector."""
    fill = {torch.uint8: 0xA5, torch.int16: 0x5A5A, torch.float32: C.SENTINEL}[dtype]
    for i, n in enumerate(C.AUX_N):
        rng = np.random.default_rng([9, rows, n])
        n_src = 2 * n + 3
        hi = 256 if dtype == torch.uint8 else 30000
        base = torch.from_numpy(rng.integers(1, hi, (rows, n_src + 13))).to(dtype).to(dev)
        src = base[:, :n_src]
        assert src.stride(0) > n_src
        idx_np = rng.integers(0, n_src, n)
        idx_np[rng.random(n) < 0.1] = -1
        if n > 1:
            idx_np[n // 2] = -1
        idx_np[-1] = n_src - 1 if n > 1 else idx_np[-1]
        idx = torch.from_numpy(idx_np).to(dev)
        out = torch.full((rows, n + C.AUX_PAD[i % 2]), fill, dtype=dtype, device=dev)
        K.gather(src, idx, out=out)
        ref = src.cpu()[:, idx.cpu().clamp(min=0)]
        ref[:, idx.cpu() < 0] = 0
        assert torch.equal(out.cpu()[:, :n], ref), (n, rows)
        assert pad_untouched(out.cpu(), n, fill)
