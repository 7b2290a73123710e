"""The lo-half split of m = 2^E in the matrix-core GP loop (csrc/kf_gp_mfma.h
gpm_exp_split): the default (f32 residual, packed round-to-nearest-even
conversion) against the split it replaced (Variant.MIXLO_SPLIT: the rounded
f16 result straight from the FMA).  The two must give the same f16 bits for
every m -- element by element through the test kernel, and through the JRC-TIP
LDS-table kernel and the 10-parameter global-table kernel in both analysis
forms, where every output must be bit-identical."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.engine.bands import DeviceBand, RecordCache, build_table
from kafka_inferenceengine_amd.ops import kernels as K
from kafka_inferenceengine_amd.utils.blocks import ntri, pack_matrix

import kernel_cases as C
from test_oracles import prosail_problem
from test_split_model import boundary_values, split_model

pytestmark = pytest.mark.gpu

N = 3 * 64 + 5            # three whole waves and a tail of 5 lanes
T = 40                    # two 32-point chunks: the peeled first chunk and the loop body
CLOUD = slice(64, 128)    # wave 1: no observation in any band
MODES = ("plain", "cancelling", "far")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def assert_same(a, b, tag):
    assert a.keys() == b.keys()
    for key in a:
        assert np.array_equal(bits(a[key]), bits(b[key])), (tag, key)


def with_variant(variant, fn):
    old = K.DEFAULT_VARIANT
    K.DEFAULT_VARIANT = variant
    try:
        return fn()
    finally:
        K.DEFAULT_VARIANT = old


# ------------------------------------------------------------------ element level
def test_split_elements_bit_identical_and_match_model(cuda):
    # E in [-40, 14] densely, the f16 subnormal / underflow boundaries and their
    # neighbours, and exponents whose m is a float32 subnormal or 0
    e = np.concatenate([np.linspace(-40.0, 14.0, 1 << 20, dtype=np.float32),
                        np.log2(boundary_values()[1:].astype(np.float64)).astype(np.float32),
                        np.array([-14, -15, -24, -25, -26, -126, -127, -140, -149, -150, -200, 14, 13.999999, 0],
                                 dtype=np.float32)])
    for v in (-14.0, -24.0, -25.0):
        x = np.float32(v)
        e = np.concatenate([e, np.array([np.nextafter(x, np.float32(0)), np.nextafter(x, np.float32(-100))])])
    et = torch.from_numpy(e).to(cuda)
    h0, l0, m0 = (t.cpu().numpy() for t in K.exp_split_probe(et, mixlo=False))
    h1, l1, m1 = (t.cpu().numpy() for t in K.exp_split_probe(et, mixlo=True))
    assert np.array_equal(bits(m0), bits(m1))
    assert np.array_equal(bits(h0), bits(h1))
    assert np.array_equal(bits(l0), bits(l1))
    # the kernel's own m through the NumPy model of the split
    assert np.isfinite(m0).all() and m0.max() <= 2.0 ** 14 and (m0 == 0).any() and (m0 >= 2.0 ** 13).any()
    hi, lo = split_model(m0)
    assert np.array_equal(bits(h0), bits(hi))
    assert np.array_equal(bits(l0), bits(lo))
    # every range of the split was visited: normal hi, subnormal hi, hi = 0 with lo != 0, both 0
    assert ((hi.astype(np.float32) > 0) & (hi.astype(np.float32) < 2.0 ** -14)).any()
    assert ((bits(hi) == 0) & (bits(lo) != 0)).any() and ((bits(hi) == 0) & (bits(lo) == 0)).any()
    assert (bits(lo) != 0).sum() > e.size // 2


# ------------------------------------------------------------------ problems
def _spread(x, centre, seed):
    """States from the centre out to far outside the training box, mixed within every wave: m from its
    largest values down through the f16 subnormals to exact 0."""
    rng = np.random.default_rng(seed)
    f = rng.permutation(np.linspace(0.0, 12.0, x.shape[0]))
    return centre[None, :] + (x - centre[None, :]) * f[:, None]


def tip_prob(mode, seed=5):
    prob = C.tip_problem(N=N, seed=seed, n_train=T, dn16=True, mask_frac=0.15)
    for r in prob["raw"]:
        r["dn"][CLOUD] = 0
    if mode == "cancelling":   # near-interpolating emulators: the lo half carries the result
        ems = k.make_tip_emulators(n_train=T, seed=seed, noise=1e-5)
        prob = dict(prob, ems=ems, specs=[k.gp_spec(ems[b], k.TIP_BAND_MAPPER[b]) for b in range(2)])
    if mode == "far":
        prob = dict(prob, x=_spread(prob["x"], k.tip_prior()[0], seed))
    return prob


def tip_table(prob, dev):
    tab = C.table(prob, dev)
    assert tab.gpm_frags > 0 and tab.layout == K.BAND_LAYOUT_TIP
    return tab


def prosail_prob(mode, seed=21):
    prob = prosail_problem(N=N, n_bands=10, seed=seed, n_train=T)
    if mode == "cancelling":
        ems = k.make_prosail_emulators(n_bands=10, n_train=T, seed=seed, noise=1e-5)
        prob = dict(prob, ems=ems, specs=[k.gp_spec(em, list(range(10))) for em in ems])
    if mode == "far":
        prob = dict(prob, x=_spread(prob["x"], k.sail_prior()[0], seed))
    dn = []
    for y, w in prob["obs"]:
        d = np.where(w > 0, np.clip(np.round(y / 1e-4), 1, 65535), 0).astype(np.int32)
        d[CLOUD] = 0
        dn.append(np.where(d > 32767, d - 65536, d).astype(np.int16))
    return dict(prob, dn=dn)


def prosail_table(prob, dev):
    dbs = [DeviceBand(K.OBS_DN16, dn=torch.from_numpy(d).to(dev), scale=1e-4, rel_unc=0.05, unc_floor=2.5e-3)
           for d in prob["dn"]]
    tab = build_table(prob["specs"], dbs, 10, RecordCache(), dev)
    assert tab.gpm_global and tab.gpm_frags == 0
    return tab


def problem(case, mode):
    return tip_prob(mode) if case == "tip" else prosail_prob(mode)


def table(case, prob, dev):
    return tip_table(prob, dev) if case == "tip" else prosail_table(prob, dev)


def forecast_spec(case):
    if case == "tip":
        return C.containment_spec(7)          # LAI propagated, the rest reset to the prior
    mu, _, Pi = k.sail_prior()
    return {"mode": 0, "m": np.ones(10), "q": np.zeros(10), "prop_mask": 0, "reset_mean": mu,
            "reset_cinv": pack_matrix(Pi), "blend": False}


# ------------------------------------------------------------------ launches
def info_launch(case, prob, dev, variant, fused_forecast, line=None):
    """Two fused Gauss-Newton iterations of the information form with every output the kernel writes."""
    n = prob["n"]
    tab = table(case, prob, dev)
    xo = torch.zeros((n, N), device=dev)
    ao = torch.zeros((ntri(n), N), device=dev)
    st = torch.zeros(N, dtype=torch.uint8, device=dev)
    mean = torch.zeros((n, N), device=dev)
    unc = torch.zeros((n, N), device=dev)
    part, part1 = K.partials_buffer(N, dev), K.partials_buffer(N, dev)
    if fused_forecast:
        rng = np.random.default_rng(3)
        pa = C.spd_blocks(rng, N, n, 5.0) * 0.2 + prob["Pf"]
        h = K.prop_args(n, forecast_spec(case), C.soa(prob["x"], dev), C.packed(pa, dev), fused=True)
        K.STRUCT_LAUNCHES.update(tip=0, dense=0)
        K.analysis(n, tab, None, None, None, xo, ao, None, st, part, prop=h, out=(mean, unc, None), variant=variant,
                   gn_fused=2, partials_first=part1, line=line)
        if case == "tip":
            assert K.STRUCT_LAUNCHES["tip"] == 1      # the structure-aware kernel, as the headline launch
    else:
        K.analysis(n, tab, C.soa(prob["x"], dev), C.soa(prob["xf"], dev), C.packed(prob["Pf"], dev), xo, ao, None, st,
                   part, out=(mean, unc, None), variant=variant, gn_fused=2, partials_first=part1)
    torch.cuda.synchronize()
    return dict(x=xo.cpu().numpy(), a=ao.cpu().numpy(), status=st.cpu().numpy(), mean=mean.cpu().numpy(),
                unc=unc.cpu().numpy(), norm=K.reduce_partials(part).cpu().numpy(),
                norm_first=K.reduce_partials(part1).cpu().numpy())


def gain_launch(case, prob, dev):
    n = prob["n"]
    tab = table(case, prob, dev)
    xo = torch.zeros((n, N), device=dev)
    po = torch.zeros((ntri(n), N), device=dev)
    st = torch.zeros(N, dtype=torch.uint8, device=dev)
    mean = torch.zeros((n, N), device=dev)
    unc = torch.zeros((n, N), device=dev)
    part, part1 = K.partials_buffer(N, dev), K.partials_buffer(N, dev)
    K.gain(n, tab, C.soa(prob["x"], dev), C.soa(prob["xf"], dev), C.packed(np.linalg.inv(prob["Pf"]), dev), xo, po,
           st, part, out=(mean, unc, None), gn_fused=2, partials_first=part1)
    torch.cuda.synchronize()
    return dict(x=xo.cpu().numpy(), p=po.cpu().numpy(), status=st.cpu().numpy(), mean=mean.cpu().numpy(),
                unc=unc.cpu().numpy(), norm=K.reduce_partials(part).cpu().numpy(),
                norm_first=K.reduce_partials(part1).cpu().numpy())


def observed(case, prob):
    """Pixels with an observation in some band."""
    dn = [r["dn"] for r in prob["raw"]] if case == "tip" else prob["dn"]
    return np.any([d != 0 for d in dn], axis=0)


def check_ran(case, mode, prob, r):
    """The launch did what the shapes are for: the cloudy wave skipped, the observed pixels analysed."""
    st, obs = r["status"], observed(case, prob)
    assert not obs[CLOUD].any() and obs[:64].any() and obs[128:192].any() and obs[192:].any()
    assert np.all(st[~obs] & K.ST_NO_OBS), (case, mode)
    if mode != "far":
        assert not np.any(st[obs] & K.ST_NO_OBS), (case, mode)
        assert np.isfinite(r["x"]).all() and r["norm"] > 0 and r["norm_first"] > 0


# ------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", ["tip", "prosail"])
def test_information_form_bit_identical(cuda, case, mode):
    prob = problem(case, mode)
    # the generic launch (the first date's kernel) and the fused forecast (every later date's);
    # the latter with the first iteration from the line tables and from the GP sums
    launches = [(False, None), (True, None), (True, False)]
    for fused, line in launches:
        new = info_launch(case, prob, cuda, K.Variant.DEFAULT, fused, line)
        old = info_launch(case, prob, cuda, K.Variant.MIXLO_SPLIT, fused, line)
        assert_same(new, old, (case, mode, fused, line))
        check_ran(case, mode, prob, new)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", ["tip", "prosail"])
def test_gain_form_bit_identical(cuda, case, mode):
    prob = problem(case, mode)
    new = gain_launch(case, prob, cuda)
    old = with_variant(K.Variant.MIXLO_SPLIT, lambda: gain_launch(case, prob, cuda))
    assert_same(new, old, (case, mode))
    check_ran(case, mode, prob, new)


def test_mixlo_variant_has_no_other_kernels(cuda):
    """The variant is built for DN16 observations only: a launch it has no kernel for is an error,
    not another kernel (which also shows the variant reaches the launcher)."""
    prob = C.tip_problem(N=N, seed=5, n_train=T, dn16=False)
    tab = C.table(prob, cuda)
    xo = torch.zeros((7, N), device=cuda)
    ao = torch.zeros((ntri(7), N), device=cuda)
    args = (7, tab, C.soa(prob["x"], cuda), C.soa(prob["xf"], cuda), C.packed(prob["Pf"], cuda), xo, ao)
    K.analysis(*args)
    with pytest.raises(RuntimeError):
        K.analysis(*args, variant=K.Variant.MIXLO_SPLIT)
    with pytest.raises(RuntimeError):
        with_variant(K.Variant.MIXLO_SPLIT, lambda: K.gain(7, tab, args[2], args[3],
                                                         C.packed(np.linalg.inv(prob["Pf"]), cuda), xo, ao))
