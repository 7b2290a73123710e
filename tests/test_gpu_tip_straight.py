"""The straight-line JRC-TIP kernel (kf_gp_mfma.h pixel_analysis_tip_sl, the
default for launches of the shape kf_core.h tip_sl_shape) against the
SPEC_PROP_TIP / SPEC_PROP_PF_TIP kernels it replaces (Variant.LOOPED_TIP) on
the same inputs, byte for byte; launches outside that shape keep the old
kernels; and, without a GPU, the host's shape predicate and the constant block
it fills (AnalysisArgs.tc) field by field.

The inputs are runs A (corrupted) and B (clean) of the containment problem
(kernel_cases.containment_problem): observed, cloudy and mixed waves, a band
missing, p_a = -I, NaN / inf states, states outside the line table (= outside
the domain box), re-indexed so that every N starts in the corrupted wave."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from kafka_inferenceengine_amd.ops import kernels as K

import kernel_cases as C

NS = [1, 63, 64, 65, 64 * 4 * 3 + 17]
TS = [32, 96]          # one chunk of 32 training points per band, and three
ROWS = ("none", "diag", "all")
OUTS = ("none", "alias", "mean", "idx")
DIAG_ROW = 27          # tri(7, 6, 6): the propagated parameter's diagonal entry


@functools.lru_cache(maxsize=None)
def problem(n_train):
    return C.containment_problem(n_train)


def subset(run, N):
    """N pixels of ``run`` starting at wave 1 (the corrupted one), wrapping around."""
    sel = (np.arange(N) + 64) % C.CONTAIN_N
    prob = run["prob"]
    sub = dict(prob, raw=[dict(dn=np.ascontiguousarray(r["dn"][sel])) for r in prob["raw"]], N=N)
    return dict(prob=sub, xa=run["xa"][sel], pa=run["pa"][sel])


def launch(run, device, variant, rows="all", out="mean", gn=2, line=None, order=False, x_prev=None, spec=None,
           q_pix=False, prop=True):
    """One launch with every output of the shape; CPU copies of what it wrote."""
    prob = run["prob"]
    n, N = prob["n"], prob["N"]
    tab = C.table(prob, device)
    g = torch.Generator().manual_seed(N)
    xo = torch.full((n, N), C.SENTINEL, device=device)
    ao = None if rows == "none" else torch.full((28, N), C.SENTINEL, device=device)
    st = torch.full((N,), 255, dtype=torch.uint8, device=device)
    dn = torch.full((N,), C.SENTINEL, device=device)
    part, part1 = K.partials_buffer(N, device), K.partials_buffer(N, device)
    plane = N if out == "alias" else N + 5
    unc = torch.full((n, plane), C.SENTINEL, device=device)
    mean = torch.full((n, plane), C.SENTINEL, device=device) if out in ("mean", "idx") else None
    idx = torch.randperm(plane, generator=g)[:N].to(device) if out == "idx" else None
    o = None if out == "none" else (mean, unc, idx)
    xa, pa = C.soa(run["xa"], device), C.packed(run["pa"], device)
    kw = {}
    if prop:
        qp = torch.full((n, N), C.CONTAIN_Q, device=device) if q_pix else None
        kw["prop"] = K.prop_args(n, spec or C.containment_spec(n), xa, pa, fused=True, q_pix=qp)
        x_f = pf = None
    else:
        x_f, pf = xa, pa      # first date: an explicit forecast
        x_prev = xa if x_prev is None else x_prev
    if order:
        kw["order"] = K.obs_order(tab, N, device)[0]
    K.STRUCT_LAUNCHES.update(tip=0, dense=0)
    K.TIP_SL_LAUNCHES.update(straight=0, looped=0)
    K.analysis(n, tab, x_prev, x_f, pf, xo, ao, None, st, part, out=o, variant=variant, line=line, gn_fused=gn,
               partials_first=part1 if gn == 2 else None, dn_out=dn, a_rows=(1 << DIAG_ROW) if rows == "diag" else None,
               **kw)
    torch.cuda.synchronize()
    res = dict(x=xo, a=ao, status=st, dn=dn, unc=None if o is None else unc, mean=mean, part=part[:part._kf_n],
               part1=part1[:part1._kf_n] if gn == 2 else None)
    res = {f: None if t is None else t.cpu().numpy() for f, t in res.items()}
    res["launches"] = dict(K.TIP_SL_LAUNCHES)
    return res


def same_bytes(a, b, what=""):
    for f in ("x", "a", "status", "dn", "unc", "mean", "part", "part1"):
        assert (a[f] is None) == (b[f] is None), (what, f)
        if a[f] is not None:
            assert a[f].tobytes() == b[f].tobytes(), (what, f, np.nonzero(np.atleast_2d(a[f] != b[f]).any(0))[0][:8])


def pair(run, device, what, **kw):
    got = launch(run, device, None, **kw)
    ref = launch(run, device, K.Variant.LOOPED_TIP, **kw)
    assert got["launches"] == {"straight": 1, "looped": 0}, (what, got["launches"])
    assert ref["launches"] == {"straight": 0, "looped": 1}, (what, ref["launches"])
    same_bytes(got, ref, what)
    return got


@pytest.fixture()
def one_block():
    """One workgroup: each of its four waves walks ceil(N / 256) pixel groups."""
    ext = K.ext()
    old = ext.get_max_blocks()
    ext.set_max_blocks(1)
    K._ANALYSIS_MEMO.clear()
    yield
    ext.set_max_blocks(old)
    K._ANALYSIS_MEMO.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("n_train", TS)
@pytest.mark.parametrize("N", NS)
def test_straight_line_kernel_equals_the_looped_kernel(cuda, one_block, N, n_train):
    """x, stored rows, rasters, status, dn_out and both iterations' norm
    partials, for every stored-rows mode and every output mode, on the
    corrupted run and its clean twin."""
    cp = problem(n_train)
    for key in "AB":
        run = subset(cp[key], N)
        for rows in ROWS:
            for out in OUTS:
                pair(run, cuda, (key, rows, out), rows=rows, out=out)
        # one fused iteration, no line tables (every wave on the GP sums), the observed-first order
        pair(run, cuda, (key, "gn1"), gn=1)
        pair(run, cuda, (key, "sums"), line=False)
        pair(run, cuda, (key, "order"), order=True)
    if N >= 65:
        # the cases are there: run A's health fallback (p_a = -I at lane 9, NaN state at lane 3 of the first
        # wave), a pixel without any observation, one outside the line table / domain box (N = 785 only)
        st = pair(subset(cp["A"], N), cuda, "A")["status"]
        assert st[9] == K.ST_NONSPD | K.ST_FALLBACK and (st[3] & K.ST_NONFINITE) and st[40] == K.ST_NO_OBS
        assert N < 785 or (st[C.px(3, 5)] == K.ST_OUT_OF_DOMAIN and (st[C.px(1, 0):C.px(2, 0)] == K.ST_NO_OBS).all())


@pytest.mark.gpu
def test_launches_outside_the_shape_keep_the_old_kernels(cuda):
    """First date (no forecast), x_prev set (a later per-chunk iteration), a
    per-pixel Q, two propagated parameters: the old kernels run, with the
    results of the looped variant's launch."""
    run = subset(problem(96)["B"], 64 * 4 + 17)
    n = 7
    two = dict(C.containment_spec(n), prop_mask=(1 << 6) | (1 << 2))
    x_prev = C.soa(run["xa"] + 0.01, cuda)
    for what, kw in (("first date", dict(prop=False, gn=1)), ("x_prev", dict(x_prev=x_prev, gn=1)),
                     ("q_pix", dict(q_pix=True)), ("two propagated", dict(spec=two))):
        got = launch(run, cuda, None, **kw)
        ref = launch(run, cuda, K.Variant.LOOPED_TIP, **kw)
        assert got["launches"]["straight"] == 0 and ref["launches"]["straight"] == 0, (what, got["launches"])
        same_bytes(got, ref, what)
        assert np.isfinite(got["x"]).all(), what


# ------------------------------------------------------------- host side
def _host_launch_args():
    """AnalysisArgs of a qualifying launch with CPU tensors (nothing is launched)."""
    cp = problem(32)
    run = subset(cp["B"], 70)
    prob = run["prob"]
    n, N = 7, prob["N"]
    tab = C.table(prob, "cpu")
    keep = dict(xo=torch.zeros((n, N)), ao=torch.zeros((28, N)), st=torch.zeros(N, dtype=torch.uint8),
                mean=torch.zeros((n, N + 5)), unc=torch.zeros((n, N + 5)), idx=torch.arange(N), tab=tab,
                line=torch.zeros(8))
    h = K.prop_args(n, C.containment_spec(n), C.soa(run["xa"], "cpu"), C.packed(run["pa"], "cpu"), fused=True)
    a = K.ext().AnalysisArgs()
    a.N, a.ld, a.n_bands, a.solve, a.gn_fused = N, N, 2, 1, 2
    a.fast_d, a.fast_obs, a.band_layout, a.gpm_frags = 4, K.OBS_DN16, K.BAND_LAYOUT_TIP, tab.gpm_frags
    a.bands, a.prop = tab.ptr, h.device_copy().data_ptr()
    a.x_out, a.a_out, a.status = keep["xo"].data_ptr(), keep["ao"].data_ptr(), keep["st"].data_ptr()
    a.out_mean, a.out_unc, a.out_idx, a.out_plane = keep["mean"].data_ptr(), keep["unc"].data_ptr(), \
        keep["idx"].data_ptr(), N + 5
    a.a_rows = 1 << DIAG_ROW
    a.a_struct = K.A_STRUCT_TIP | K.A_STRUCT_TIP_PRIOR
    a.dom_check, a.dom_lo, a.dom_hi = 1, list(tab.dom[0]), list(tab.dom[1])
    a.line_tab, a.line_t0, a.line_inv_h, a.line_n, a.line_j = keep["line"].data_ptr(), 0.25, 8.0, 40, 6
    return a, h, tab, keep


def test_shape_predicate():
    ext = K.ext()
    a, h, tab, keep = _host_launch_args()
    descs = list(tab.descs)
    assert tab.gpm_frags > 0 and [d.map_kind for d in descs] == [2, 3]
    assert ext.tip_sl_shape(7, a, h.args, descs)
    assert not ext.tip_sl_shape(7, a, None, descs) and not ext.tip_sl_shape(7, a, h.args, descs[:1])
    assert not ext.tip_sl_shape(10, a, h.args, descs)

    def without(**kw):
        """The predicate with fields of a / the PropArgs changed, restored afterwards."""
        objs = {k_: (h.args if k_ in ("prop_mask", "q_pix", "mode") else a) for k_ in kw}
        old = {k_: getattr(objs[k_], k_) for k_ in kw}
        for k_, v in kw.items():
            setattr(objs[k_], k_, v)
        r = ext.tip_sl_shape(7, a, h.args, descs)
        for k_, v in old.items():
            setattr(objs[k_], k_, v)
        return r

    ptr = keep["xo"].data_ptr()
    for kw in (dict(prop=0), dict(x_prev=ptr), dict(a_struct=K.A_STRUCT_TIP), dict(a_struct=0), dict(solve=0),
               dict(b_out=ptr), dict(x0_out=ptr), dict(reg_v=ptr), dict(variant=int(K.Variant.LOOPED_TIP)),
               dict(variant=int(K.Variant.MIXLO_SPLIT)), dict(fast_obs=K.OBS_F32), dict(band_layout=0),
               dict(gpm_frags=0), dict(a_in=ptr, b_in=ptr), dict(a_rows=1), dict(a_rows=(1 << DIAG_ROW) | 1),
               dict(prop_mask=0), dict(prop_mask=(1 << 6) | 1), dict(q_pix=ptr), dict(line_j=5), dict(gn_fused=3),
               dict(out_unc=0), dict(N=1 << 30, ld=1 << 30), dict(out_plane=1 << 30), dict(x_out=0)):
        assert not without(**kw), kw
    for kw in (dict(a_rows=0), dict(a_out=0), dict(out_mean=0, out_unc=0, out_idx=0), dict(out_mean=0, out_idx=0),
               dict(out_idx=0), dict(status=0), dict(line_tab=0), dict(gn_fused=1), dict(dom_check=0),
               dict(prop_mask=1 << 2, line_j=2, a_rows=1 << 13)):
        assert without(**kw), kw
    # a band with a diagnostic H0 output, or not a DN16 band
    for f, v in (("h0_out", ptr), ("obs", K.OBS_F32), ("map_kind", 0)):
        old = getattr(descs[1], f)
        setattr(descs[1], f, v)
        assert not ext.tip_sl_shape(7, a, h.args, descs), f
        setattr(descs[1], f, old)
    assert ext.tip_sl_shape(7, a, h.args, descs)


def test_constant_block_field_by_field():
    ext = K.ext()
    a, h, tab, keep = _host_launch_args()
    descs = list(tab.descs)
    assert a.tc["on"] == 0 and not a.tc_on
    assert ext.tip_const_fill(7, a, h.args, descs) and a.tc_on
    t, p = a.tc, h.args
    f32 = lambda v: [float(np.float32(x)) for x in v]   # noqa: E731
    assert (t["on"], t["j"]) == (1, 6)
    assert t["m"] == f32(p.m)[6] == 1.0 and t["q"] == f32(p.q)[6] == float(np.float32(C.CONTAIN_Q))
    assert t["xa_row"] == p.x_a + 4 * 6 * p.ld and t["pa_row"] == p.p_a + 4 * DIAG_ROW * p.ld
    assert t["mean"][:7] == f32(p.reset_mean)[:7] and t["cinv"] == f32(p.reset_cinv)[:28]
    assert any(t["mean"][:7]) and any(t["cinv"])
    assert (t["line_tab"], t["line_t0"], t["line_inv_h"], t["line_n"]) == (a.line_tab, 0.25, 8.0, 40)
    assert t["dom_check"] == 1 and t["dom_lo"][:7] == f32(a.dom_lo)[:7] and t["dom_hi"][:7] == f32(a.dom_hi)[:7]
    for b in range(2):
        c, d = t["band"][b], descs[b]
        assert c["center"] == f32(d.center)[:4] and c["coef"] == f32(d.coef)[:4] and any(c["coef"])
        assert (c["offset"], c["gpm_scale"], c["scale"], c["rel_unc"], c["unc_floor"], c["nchunk"]) == \
            (d.offset, d.gpm_scale, d.scale, d.rel_unc, d.unc_floor, d.gpm_nchunk)
        assert c["nchunk"] == 1 and c["scale"] > 0 and t["dn"][b] == d.dn != 0
    assert (t["rows"], t["out"]) == (1, 2)      # TIP_ROWS_DIAG, TIP_OUT_MEAN
    assert (t["ld"], t["out_plane"], t["gn_fused"], t["gpm_frags"]) == (a.ld, a.out_plane, 2, tab.gpm_frags)
    for f in ("x_out", "a_out", "out_mean", "out_unc", "out_idx", "status"):
        assert t[f] == getattr(a, f) != 0, f
    # the other instantiations' modes, and a launch outside the shape clears the block
    a.a_rows = 0
    a.out_mean = 0
    a.out_idx = 0
    assert ext.tip_const_fill(7, a, h.args, descs) and (a.tc["rows"], a.tc["out"]) == (2, 1)
    a.a_out = 0
    a.out_unc = 0
    assert ext.tip_const_fill(7, a, h.args, descs) and (a.tc["rows"], a.tc["out"]) == (0, 0)
    a.b_out = keep["xo"].data_ptr()
    assert not ext.tip_const_fill(7, a, h.args, descs) and a.tc["on"] == 0 and a.tc["x_out"] == 0
