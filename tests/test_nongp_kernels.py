"""The analysis and gain kernels that are not Gaussian-process kernels, row by row of the launch tables
(csrc/kf_device.h KF_K1_ROWS_ANY, KF_K1G_ROWS_SMALL), against a float64 model that shares no code with
kf_core.h:

* ``analysis_kernel<NP, FD_LINEAR | FD_PRECOMP, OBS>``: 6 state sizes x 2 operators x 4 encodings;
* ``analysis_kernel<NP, 0, 0>`` with bands that differ in operator and encoding, and ``gain_kernel<NP, 0, 0>``.

The observation bands are built from raw bits (uint16 DN, float32, bf16 patterns); ``kernel_cases.decode_model``
is the float64 model of ``decode_obs`` (and ``DeviceBand.decode`` is held to it), the operators are evaluated in
float64 NumPy (offset + x . c, the stored precomputed rows, ``sar_observation_operator``, ``emulator.predict``),
the analysis is ``inference.analysis_blocks`` / ``gain_blocks`` over the float32-rounded inputs and the status
byte is ``kernel_cases.info_model`` / ``gain_model``.  Every SoA operand has a leading dimension larger than N
(``kernel_cases.AUX_PAD``) and every output is checked to keep its sentinel in the padding columns.  N runs over
``kernel_cases.AUX_N``: below a wave, around a wave, two workgroups and a pixel.

Each test runs on the CPU (the host runner: it validates the inputs and the model) and, marked ``gpu``, on the
MI355X, where each launch must also take the expected line of ``ext.launch_table()``.

Coverage condition (``kernel_cases.coverage``): every 64-pixel block of a case holds an observed and an
unobserved pixel.  A block of one pixel (N = 1, and the last pixel of N = 65 and 513) cannot hold both: there the
pixel is observed, so the tail lane does real work.

Exact: status bytes, plan names, the padding sentinels and the bit equalities of the two-iteration shortcut.

A: max |A - A_r| / sqrt(A_ii A_jj) <= 1e-6 for linear and precomputed bands (at most four f32 rank-one terms on
the forecast precision) and <= 1e-4 for launches with GP or SAR Jacobians (the bound of test_oracles.py).

x, information form: per pixel |x - x_r|_inf / ((|x_r|_inf + 0.05) cond_2(A_r)) in units of 2^-24: the f32
solve's error follows the pixel's conditioning (a planted DN of 1 weighs 1.6e5).  x and P, gain form: P entries
scaled by sqrt(Pf_ii Pf_jj) and x by sqrt(Pf_jj) + 0.05 (the error scales with the operands of the subtraction),
in units of 2^-24.  The limits are 4 x the worst value of the host runner (the same per-pixel source; the device
differs in rcp, sqrt and FMA contraction, not in algorithm) over all cases of the group:

    measure                                        host runner   limit    MI355X
    ---------------------------------------------  -----------   ------   -------
    x, linear / precomputed rows (info)            9.31          37.2     10.52
    x, GP / SAR mixed launch (info)                12.18         48.7     13.29
    A, linear / precomputed rows                   2.48e-7       1e-6     2.55e-7
    A, GP / SAR mixed launch                       1.63e-5       1e-4     1.63e-5
    x, gain form                                   2578.16       10313    2578.16
    x, gain form, outside the all-band edge run    224.04        896      224.04
    P, gain form                                   58.66         235      58.66
    x, gain form, GP / SAR mixed launch            259.33        1037     205.99
    P, gain form, GP / SAR mixed launch            83.99         336      83.99

The gain form's worst x is one pixel: the planted BF16Y y = 0 in all four bands of a 4-parameter state (w = 1.6e5
each, the state moves 25 forecast standard deviations); pixels 1 .. 10, where every band carries the same decode
edge, are therefore also held to a second limit without them.  The smallest eigenvalue of the Joseph form's
scaled P at the strongly observed pixels is 145.77 units on both (never negative).

The Joseph form must meet the gain bounds too and, at the strongly observed pixels (``gain_model``: the update
removes all but 1e-2 of the forecast variance along h), the smallest eigenvalue of its scaled P must be >= -n
times the P limit (an elementwise error t moves an eigenvalue of an n x n matrix by at most n t).

h0_out: exactly the stored pre_h0 for a precomputed band; for a linear band within (n + 1) 2^-24 (|offset| +
sum |c_j x_j|), one rounding per fused multiply-add of the dot product.  dn_out: with e the pixel's x limit above
as an absolute error, |dn - dn_r| <= 2 |d_r|_1 e + n e^2 + (n + 2) 2^-24 dn_r for d = x - x0.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from kafka_inferenceengine_amd.ops import kernels as K
from kafka_inferenceengine_amd.utils.blocks import ntri, pack_blocks, unpack_blocks

import kernel_cases as C

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
U = 2.0 ** -24
A_TOL, A_TOL_MIXED = 1e-6, 1e-4
# 4 x the host runner's worst value (module docstring), in units of 2^-24
X_LIMIT, X_LIMIT_MIXED = 4 * 9.31, 4 * 12.18
GAIN_X_LIMIT, GAIN_X_REST_LIMIT, GAIN_P_LIMIT = 4 * 2578.16, 4 * 224.04, 4 * 58.66
GAIN_X_LIMIT_MIXED, GAIN_X_REST_LIMIT_MIXED, GAIN_P_LIMIT_MIXED = 4 * 259.33, 4 * 259.33, 4 * 83.99
OPS = {"linear": K.FD_LINEAR, "precomp": K.FD_PRECOMP}


@pytest.fixture(params=DEVICES)
def dev(request):
    if request.param == "cuda":
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        return torch.device("cuda", 0)
    return torch.device("cpu")


# ------------------------------------------------------------------ cases
def n_bands(n, enc):
    return 2 + (n + enc) % 3


def row_bands(n, op, enc):
    return ((op, enc),) * n_bands(n, enc)


def mixed_bands(n):
    """Bands that differ in operator and encoding (n <= 3) or in encoding alone (n >= 4): fast_d = 0."""
    lin, sar, gp, pre = ("linear", K.OBS_DN16), ("sar", K.OBS_F32), ("gp", K.OBS_BF16), ("precomp", K.OBS_BF16Y)
    if n >= 4:
        return tuple(("linear", e) for e in C.ENCODINGS)
    return {1: (lin, pre), 2: (sar, lin, pre), 3: (lin, sar, gp, pre)}[n]


def has_gp_or_sar(bands):
    return any(op in ("gp", "sar") for op, _ in bands)


# the (NP, operator) whose launch sweeps every N of the encoding; the others run at N = 65 and 513
SWEEP = {K.OBS_DN16: (1, "linear"), K.OBS_F32: (2, "precomp"), K.OBS_BF16: (3, "linear"), K.OBS_BF16Y: (4, "precomp")}


def shapes(n, op, enc):
    ns = C.AUX_N if SWEEP[enc] == (n, op) else (65, 513)
    return [(N, C.AUX_PAD[(i + n) % 2]) for i, N in enumerate(ns)]


def fast_name(n, op, enc):
    return f"analysis_kernel<{n}, {OPS[op]}, {enc}, 4, false>"


def generic_name(n):
    return f"analysis_kernel<{n}, 0, 0, 4, false>"


def gain_name(n):
    return f"gain_kernel<{n}, 0, 0>"


ROWS = [(n, op, enc) for n in C.AUX_NP for op in OPS for enc in C.ENCODINGS]
ROW_IDS = [f"{n}-{op}-{C.ENC_NAME[enc]}" for n, op, enc in ROWS]
# one encoding and operator per state size, for the tests that run "at every NP"
PER_NP = [(n, C.ENCODINGS[i % 4]) for i, n in enumerate(C.AUX_NP)]
GAIN_TABLES = ("linear", "precomp", "mixed")


def expected_names():
    """The table lines the device half of this module launches (each test asserts the line it took)."""
    return ({fast_name(*r) for r in ROWS} | {generic_name(n) for n in C.AUX_NP} | {gain_name(n) for n in C.AUX_NP})


# ------------------------------------------------------------------ launches
def pad_untouched(t, N, fill=C.SENTINEL):
    tail = t[..., N:]
    return tail.numel() > 0 and torch.equal(tail, torch.full_like(tail, fill))


def sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def launch(c, dev, pad, fast=True, gn_fused=1, h0=False, dn=False, norms=False, fused=False, bands=None, solve=True,
           chain=None):
    """One K.analysis launch of the case with sentinel-filled outputs of leading dimension N + pad; -> dict of
    CPU tensors ([rows, ld] / [ld]), the norms and the plan (None on the host runner)."""
    n, N = c["n"], c["N"]
    ld, nt = N + pad, ntri(n)
    tab, h0o = C.nongp_table(c, dev, pad, h0_out=h0, bands=bands)
    xo = C.sentinel(n, ld, dev) if solve else None
    ao = C.sentinel(nt, ld, dev)
    bo = None if solve else C.sentinel(n, ld, dev)
    st = torch.full((ld,), C.STATUS_FILL, dtype=torch.uint8, device=dev)
    dno = C.sentinel(1, ld, dev)[0] if dn else None
    part = K.partials_buffer(N, dev) if norms else None
    part1 = K.partials_buffer(N, dev) if norms and gn_fused == 2 else None
    a_in, b_in = (None, None) if chain is None else (chain["a"].to(dev), chain["b"].to(dev))
    K.LAST_PLAN = None
    if fused:
        prop = K.prop_args(n, c["spec"], C.padded(c["xa"].T, ld, dev), C.padded(pack_blocks(c["pa"]), ld, dev), N=N,
                           fused=True)
        K.analysis(n, tab, None, None, None, xo, ao, None, st, part, N=N, fast=fast, prop=prop, dn_out=dno)
    else:
        K.analysis(n, tab, C.padded(c["x0"].T, ld, dev), C.padded(c["xf"].T, ld, dev),
                   C.padded(pack_blocks(c["Pf"]), ld, dev), xo, ao, bo, st, part, N=N, solve=solve, fast=fast,
                   a_in=a_in, b_in=b_in, gn_fused=gn_fused, partials_first=part1, dn_out=dno)
    sync(dev)
    r = dict(table=tab, plan=K.LAST_PLAN, a=ao.cpu(), status=st.cpu(), x=None if xo is None else xo.cpu(),
             b=None if bo is None else bo.cpu(), dn=None if dno is None else dno.cpu(),
             h0=None if h0o is None else [t.cpu() for t in h0o])
    if norms:
        r["norm"] = float(K.reduce_partials(part).cpu())
        r["norm_first"] = None if part1 is None else float(K.reduce_partials(part1).cpu())
    for key in ("x", "a", "b", "dn"):
        assert r[key] is None or pad_untouched(r[key], N), f"{key}: wrote past N"
    assert all(pad_untouched(t, N) for t in r["h0"] or []), "h0_out: wrote past N"
    assert pad_untouched(r["status"], N, C.STATUS_FILL), "status: wrote past N"
    return r


_MODELS: dict = {}


def model_of(c, tab, bands=None):
    """info_model of the case (built once; the GP domain box comes from the band table)."""
    key = (id(c), None if bands is None else tuple(bands))
    if key not in _MODELS:
        ev = c["evals"] if bands is None else [c["evals"][i] for i in bands]
        _MODELS[key] = (c, C.info_model(c["x0"], c["xf"], c["Pf"], ev, dom=tab.dom))
    return _MODELS[key][1]


def a_err(A, Ar):
    d = np.sqrt(np.einsum("nii->ni", Ar))
    return float(np.max(np.abs(A - Ar) / (d[:, :, None] * d[:, None, :])))


def x_units(x, m):
    """Per pixel |x - x_r|_inf / ((|x_r|_inf + 0.05) cond_2(A_r)) in units of 2^-24; -> (worst, scale [N])."""
    scale = (np.abs(m["x"]).max(1) + 0.05) * np.linalg.cond(m["A"])
    return float(np.max(np.abs(x - m["x"]).max(1) / scale)) / U, scale


def check_info(c, r, m, label, dev, mixed=False):
    """x, the full packed A and the status byte of launch ``r`` against the model ``m``."""
    n, N = c["n"], c["N"]
    assert C.coverage(c), "a 64-pixel block without an observed or without an unobserved pixel"
    assert np.array_equal(r["status"][:N].numpy(), m["status"]), (label, r["status"][:N].numpy() ^ m["status"])
    ea = a_err(unpack_blocks(r["a"][:, :N].numpy().astype(np.float64), n), m["A"])
    ex, _ = x_units(r["x"][:, :N].numpy().T.astype(np.float64), m)
    print(f"MEASURE {'mixed' if mixed else 'plain'} {dev.type} x {ex:.2f} A {ea:.2e}  [{label} N={N}]")
    assert ea <= (A_TOL_MIXED if mixed else A_TOL), (label, N, ea)
    assert ex <= (X_LIMIT_MIXED if mixed else X_LIMIT), (label, N, ex)


def check_plan(r, dev, name):
    if dev.type == "cuda":
        assert r["plan"] is not None and r["plan"]["name"] == name, (r["plan"], name)


# ------------------------------------------------------------------ the decode model's host twin
@pytest.mark.parametrize("enc", C.ENCODINGS, ids=[C.ENC_NAME[e] for e in C.ENCODINGS])
def test_device_band_decode_agrees_with_the_decode_model(dev, enc):
    """DeviceBand.decode (float32 torch, the documented host twin of decode_obs) on the planted edges: the same
    pixels kept, y exact, w within float32 rounding of the float64 weight."""
    c = C.nongp_case(3, 65, row_bands(3, "linear", enc))
    for b, raw in enumerate(c["raws"]):
        y, w = C.device_band(enc, raw, 65, dev).decode()
        ym, wm = C.decode_model(enc, raw)
        y, w = y.cpu().numpy().astype(np.float64), w.cpu().numpy().astype(np.float64)
        assert np.array_equal(w > 0, wm > 0) and np.isfinite(w).all() and np.isfinite(y).all(), b
        assert np.array_equal(y, ym), b
        assert np.allclose(w, wm, rtol=4.01 * U, atol=0.0), (b, np.max(np.abs(w - wm) / np.maximum(wm, 1e-30)))
        kinds = {bool(v) for v in wm > 0}
        assert kinds == {True, False}


# ------------------------------------------------------------------ 1. every specialised row
@pytest.mark.parametrize("n,op,enc", ROWS, ids=ROW_IDS)
def test_specialised_row_vs_float64_model(dev, n, op, enc):
    """analysis_kernel<NP, FD_LINEAR | FD_PRECOMP, OBS>: x, A and the status byte with the decode edges, a pixel
    with every band masked, one masked through the mask plane alone and (precomputed) NaN / Inf operator rows."""
    for N, pad in shapes(n, op, enc):
        c = C.nongp_case(n, N, row_bands(n, op, enc))
        r = launch(c, dev, pad)
        assert r["table"].fast_d == OPS[op] and r["table"].fast_obs == enc
        check_plan(r, dev, fast_name(n, op, enc))
        m = model_of(c, r["table"])
        if N >= 63:
            assert (m["status"] & K.ST_NO_OBS).any() and (op == "linear" or (m["status"] & K.ST_BAD_OP).any())
        check_info(c, r, m, fast_name(n, op, enc), dev)


# ------------------------------------------------------------------ 2. h0_out, dn_out, b_out
H0_ROWS = [(1, "precomp", K.OBS_DN16), (2, "linear", K.OBS_DN16), (3, "precomp", K.OBS_F32),
           (4, "linear", K.OBS_BF16Y), (7, "precomp", K.OBS_BF16), (10, "linear", K.OBS_F32)]


@pytest.mark.parametrize("n,op,enc", H0_ROWS, ids=[f"{n}-{op}-{C.ENC_NAME[e]}" for n, op, e in H0_ROWS])
def test_h0_out_and_dn_out_vs_model(dev, n, op, enc):
    """The diagnostics planes: h0_out per band (0 where the band is unobserved, H0 where it is) and dn_out
    (|x - x0|^2 per pixel), each in a launch of its own."""
    for N, pad in ((65, C.AUX_PAD[0]), (513, C.AUX_PAD[1])):
        c = C.nongp_case(n, N, row_bands(n, op, enc))
        r = launch(c, dev, pad, h0=True)
        check_plan(r, dev, fast_name(n, op, enc))
        m = model_of(c, r["table"])
        check_info(c, r, m, "h0_out " + fast_name(n, op, enc), dev)
        for b, (H0, h, y, w) in enumerate(c["evals"]):
            got = r["h0"][b][:N].numpy().astype(np.float64)
            ref = np.where(w > 0, H0, 0.0)
            if op == "precomp":
                assert np.array_equal(got, ref, equal_nan=True), b
            else:
                bound = (n + 1) * U * (abs(c["specs"][b].offset) + np.abs(h * c["x0"]).sum(1))
                assert np.all(np.abs(got - ref) <= bound), (b, float(np.max(np.abs(got - ref) / bound)))
        r = launch(c, dev, pad, dn=True, norms=True)
        check_info(c, r, m, "dn_out " + fast_name(n, op, enc), dev)
        _, scale = x_units(m["x"], m)
        d = m["x"] - c["x0"]
        dn_r = (d * d).sum(1)
        e = X_LIMIT * U * scale
        bound = 2 * np.abs(d).sum(1) * e + n * e * e + (n + 2) * U * dn_r
        got = r["dn"][:N].numpy().astype(np.float64)
        assert np.all(np.abs(got - dn_r) <= bound), float(np.max(np.abs(got - dn_r) / bound))
        # the launch's norm is the f64 sum of the per-pixel values it wrote
        assert abs(r["norm"] - got.sum()) <= 1e-12 * got.sum()


@pytest.mark.parametrize("n,enc", [(4, K.OBS_F32), (7, K.OBS_BF16Y)], ids=["4-f32", "7-bf16y"])
def test_precomputed_band_chunks_chained_through_b_out(dev, n, enc):
    """solve=False with b_out on an FD_PRECOMP row, continued by a second chunk through a_in / b_in: the split GP
    path's accumulation at state sizes other than 10."""
    bands = (("precomp", enc),) * 4
    for N, pad in ((65, C.AUX_PAD[1]), (513, C.AUX_PAD[0])):
        c = C.nongp_case(n, N, bands)
        assert C.coverage(c)
        r1 = launch(c, dev, pad, bands=(0, 1), solve=False)
        check_plan(r1, dev, fast_name(n, "precomp", enc))
        r2 = launch(c, dev, pad, bands=(2, 3), chain=r1)
        check_plan(r2, dev, fast_name(n, "precomp", enc))
        m = model_of(c, r2["table"])
        flags = K.ST_BAD_OP | K.ST_NO_OBS
        for r, idx in ((r1, (0, 1)), (r2, (2, 3))):
            mc = model_of(c, r["table"], idx)
            assert np.array_equal(r["status"][:N].numpy() & flags, mc["status"] & flags), idx
        ea = a_err(unpack_blocks(r2["a"][:, :N].numpy().astype(np.float64), n), m["A"])
        ex, _ = x_units(r2["x"][:, :N].numpy().T.astype(np.float64), m)
        print(f"MEASURE plain {dev.type} x {ex:.2f} A {ea:.2e}  [chained precomp {n} N={N}]")
        assert ea <= A_TOL and ex <= X_LIMIT, (ea, ex)


# ------------------------------------------------------------------ 3. the linear two-iteration shortcut
@pytest.mark.parametrize("n,enc", PER_NP, ids=[f"{n}-{C.ENC_NAME[e]}" for n, e in PER_NP])
def test_linear_second_iteration_reproduces_the_first(dev, n, enc):
    """gn_fused = 2 on an FD_LINEAR row ends after the first iteration (kf_core.h lin2); on the generic row the
    second iteration runs and must reproduce the first bit for bit: x, A, status equal to the single-iteration
    launch, the second norm exactly 0 and the first bit-equal to the single iteration's."""
    for N, pad, fast in ((65, C.AUX_PAD[0], True), (513, C.AUX_PAD[1], True), (65, C.AUX_PAD[1], False),
                         (513, C.AUX_PAD[0], False)):
        c = C.nongp_case(n, N, row_bands(n, "linear", enc))
        name = fast_name(n, "linear", enc) if fast else generic_name(n)
        r2 = launch(c, dev, pad, fast=fast, gn_fused=2, norms=True)
        r1 = launch(c, dev, pad, fast=fast, gn_fused=1, norms=True)
        for r in (r1, r2):
            check_plan(r, dev, name)
        check_info(c, r1, model_of(c, r1["table"]), "gn_fused " + name, dev)
        for key in ("x", "a", "status"):
            assert torch.equal(r1[key].view(torch.uint8), r2[key].view(torch.uint8)), (name, key)
        assert r2["norm"] == 0.0, (name, r2["norm"])
        assert r1["norm"] > 0.0 and r2["norm_first"] == r1["norm"], (name, r2["norm_first"], r1["norm"])


# ------------------------------------------------------------------ 4. the generic kernel, mixed bands
@pytest.mark.parametrize("n", C.AUX_NP)
def test_generic_kernel_with_mixed_bands(dev, n):
    """analysis_kernel<NP, 0, 0>: linear / DN16, SAR / F32 (per-pixel angle), GP / BF16 and precomputed / BF16Y
    bands in one launch (NP <= 3), linear bands in the four encodings (NP >= 4)."""
    bands = mixed_bands(n)
    for N, pad in ((65, C.AUX_PAD[0]), (513, C.AUX_PAD[1])):
        c = C.nongp_case(n, N, bands)
        r = launch(c, dev, pad)
        assert r["table"].fast_d == 0
        check_plan(r, dev, generic_name(n))
        check_info(c, r, model_of(c, r["table"]), "mixed " + generic_name(n), dev, mixed=has_gp_or_sar(bands))


# ------------------------------------------------------------------ 5. gain form
def gain_launch(c, dev, pad, joseph):
    n, N = c["n"], c["N"]
    ld = N + pad
    tab, _ = C.nongp_table(c, dev, pad)
    xo, po = C.sentinel(n, ld, dev), C.sentinel(ntri(n), ld, dev)
    st = torch.full((ld,), C.STATUS_FILL, dtype=torch.uint8, device=dev)
    ext, plans = K.ext(), []
    real = ext.gain

    def recording(np_, a, *rest):
        plans.append(ext.gain_plan(np_, a))
        return real(np_, a, *rest)

    ext.gain = recording
    try:
        K.gain(n, tab, C.padded(c["x0"].T, ld, dev), C.padded(c["xf"].T, ld, dev),
               C.padded(pack_blocks(c["Pcov"]), ld, dev), xo, po, st, N=N, joseph=joseph)
    finally:
        ext.gain = real
    sync(dev)
    xo, po, st = xo.cpu(), po.cpu(), st.cpu()
    assert pad_untouched(xo, N) and pad_untouched(po, N) and pad_untouched(st, N, C.STATUS_FILL)
    return plans[-1], xo[:, :N].numpy().T.astype(np.float64), \
        unpack_blocks(po[:, :N].numpy().astype(np.float64), n), st[:N].numpy()


@pytest.mark.parametrize("table", GAIN_TABLES)
@pytest.mark.parametrize("n,enc", PER_NP, ids=[f"{n}-{C.ENC_NAME[e]}" for n, e in PER_NP])
def test_gain_form_plain_and_joseph_vs_gain_blocks(dev, n, enc, table):
    """gain_kernel<NP, 0, 0> over the linear, precomputed and mixed tables, plain and Joseph form."""
    bands = mixed_bands(n) if table == "mixed" else row_bands(n, table, enc)
    for N, pad in ((65, C.AUX_PAD[1]), (513, C.AUX_PAD[0])):
        c = C.nongp_case(n, N, bands)
        assert C.coverage(c)
        m = C.gain_model(c)
        assert m["strong"].any()
        mixed = has_gp_or_sar(bands)
        lim_x, lim_rest, lim_p = (GAIN_X_LIMIT_MIXED, GAIN_X_REST_LIMIT_MIXED, GAIN_P_LIMIT_MIXED) if mixed else \
            (GAIN_X_LIMIT, GAIN_X_REST_LIMIT, GAIN_P_LIMIT)
        # the pixels outside the run where every band carries the same decode edge
        rest = np.ones(N, bool)
        rest[C.EDGE_ALL:C.EDGE_ALL + max(len(e) for e in C.DECODE_EDGES.values())] = False
        sd = np.sqrt(np.einsum("nii->ni", c["Pcov"]))
        for joseph in (False, True):
            plan, x, P, st = gain_launch(c, dev, pad, joseph)
            assert plan["name"] == gain_name(n), plan
            assert np.array_equal(st, m["status"]), (joseph, st ^ m["status"])
            ex_px = (np.abs(x - m["x"]) / (sd + 0.05)).max(1) / U
            ex, ex_rest = float(ex_px.max()), float(ex_px[rest].max())
            ep = float(np.max(np.abs(P - m["P"]) / (sd[:, :, None] * sd[:, None, :]))) / U
            S = P[m["strong"]] / (sd[:, :, None] * sd[:, None, :])[m["strong"]]
            eig = float(np.linalg.eigvalsh(S).min()) / U
            print(f"MEASURE {'gainmixed' if mixed else 'gain'} {dev.type} x {ex:.2f} xrest {ex_rest:.2f} P {ep:.2f} "
                  f"eig {eig:.2f}  "
                  f"[{table} {gain_name(n)} N={N} joseph={joseph}]")
            assert ex <= lim_x and ex_rest <= lim_rest and ep <= lim_p, (joseph, ex, ex_rest, ep)
            if joseph:
                assert eig >= -n * lim_p, eig


# ------------------------------------------------------------------ 6. fused forecast on the specialised rows
@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("n,enc", [(3, K.OBS_DN16), (7, K.OBS_BF16)], ids=["3-dn16", "7-bf16"])
def test_fused_forecast_on_the_specialised_rows(dev, n, enc, op):
    """analysis(prop=...) on an FD_LINEAR and an FD_PRECOMP row, one propagated parameter, linearised at the
    forecast: the arm where the correction form (precomputed: prior part exactly 0) and the absolute form
    (linear: P_f^-1 x_f) differ."""
    for N, pad in ((65, C.AUX_PAD[0]), (513, C.AUX_PAD[1])):
        c = C.nongp_case(n, N, row_bands(n, op, enc), fused=True)
        r = launch(c, dev, pad, fused=True)
        check_plan(r, dev, fast_name(n, op, enc))
        check_info(c, r, model_of(c, r["table"]), "fused " + fast_name(n, op, enc), dev)


# ------------------------------------------------------------------ the rows this module launches
def test_every_non_gp_row_of_the_launch_table_is_launched():
    """ext.launch_table() minus the lines the tests above launch (and assert, on the device) holds no
    analysis_kernel<*, -1, *>, <*, -2, *>, <*, 0, 0> and no gain_kernel<*, 0, 0> line."""
    import re
    names = expected_names()
    table = set(K.ext().launch_table())
    assert names <= table, sorted(names - table)
    left = [t for t in table - names
            if re.match(r"analysis_kernel<\d+, (-1|-2), \d+,", t) or re.match(r"analysis_kernel<\d+, 0, 0,", t)
            or re.match(r"gain_kernel<\d+, 0, 0>", t)]
    assert not left, sorted(left)
    assert len(names) == 60
