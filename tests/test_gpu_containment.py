"""Per-pixel fault containment on the matrix-core kernels (kf_gp_mfma.h): a
pixel is a lane of a wave that cooperates through MFMA operands, lane swaps
and wave votes, so a sick pixel -- NaN, inf, an indefinite precision, no
observation -- must stay in its lane: every other pixel's bits equal those of
the clean twin of the launch, the sick one carries the status byte the
float64 classifier (kernel_cases.info_model) gives it and keeps its forecast,
and the date's norm stays finite.  The same runs on the host runner (no GPU
needed) check the classifier and the shared epilogue."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.engine.bands import RecordCache, build_table
from kafka_inferenceengine_amd.inference import gain_blocks
from kafka_inferenceengine_amd.ops import kernels as K
from kafka_inferenceengine_amd.utils.blocks import ntri, pack_blocks, unpack_blocks

import kernel_cases as C
from kernel_cases import px
from test_oracles import dbands, prosail_problem, x_err

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
N_TRAIN = [33, 160]      # SPEC_PROP_PF_TIP (small emulators) and SPEC_PROP_TIP (the headline kernel)
BAD = K.ST_NONSPD | K.ST_FALLBACK


@pytest.fixture(params=DEVICES)
def dev(request):
    if request.param == "cuda":
        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        return torch.device("cuda", 0)
    return torch.device("cpu")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(a, b, sel, what):
    for f in what:
        fa, fb = a[f], b[f]
        if isinstance(fa, list):
            for i, (u, v) in enumerate(zip(fa, fb)):
                assert np.array_equal(bits(u)[..., sel], bits(v)[..., sel]), (f, i)
        elif fa.dtype == np.uint8:
            assert np.array_equal(fa[sel], fb[sel]), (f, np.nonzero(fa != fb)[0])
        else:
            d = np.nonzero((bits(fa) != bits(fb)).any(0) & sel)[0]
            assert d.size == 0, (f, d)


@functools.lru_cache(maxsize=None)
def problem(n_train, spatial=False):
    return C.containment_problem(n_train, spatial=spatial)


@functools.lru_cache(maxsize=None)
def launched(n_train, device, key, variant=None, line=None):
    """One launch of run ``key`` of the shared problem (computed once, read only)."""
    r = C.containment_launch(problem(n_train)[key], torch.device(device), variant=variant, line=line)
    if device != "cpu" and variant is None:
        # the structure-aware kernel ran (SPEC_PROP_PF_TIP / SPEC_PROP_TIP)
        assert r["launches"] == {"tip": 1, "dense": 0}, r["launches"]
    return r


@functools.lru_cache(maxsize=None)
def model(n_train, key, host):
    """The float64 model of run ``key``; ``host``: the host runner's right-hand side."""
    dom = launched(n_train, "cpu", key)["dom"]
    return C.containment_model(problem(n_train)[key], dom=dom, prior_product=host)


OUT = ("x", "a", "status", "mean", "unc", "h0")


def contained(a, b, b_sums, cp, what=OUT):
    """A's uncorrupted pixels have the clean twin's bits.  Wave 1 of A holds
    observed lanes whose propagated parameter is NaN / inf, so the wave takes
    the GP sums where the twin's takes the line tables (last bits of H0): its
    pixels are compared with the twin launched without line tables (``b_sums``:
    every wave on the GP sums), which also shows that the wave left the tables;
    every other wave with the twin as launched."""
    w1 = np.zeros(cp["N"], bool)
    w1[px(1, 0):px(2, 0)] = True
    same_bits(a, b, ~cp["corrupt"] & ~w1, what)
    same_bits(a, b_sums, ~cp["corrupt"] & w1, what)


# ------------------------------------------------------- information form
@pytest.mark.parametrize("n_train", N_TRAIN)
def test_uncorrupted_pixels_equal_the_clean_twin(dev, n_train):
    """Every pixel whose own inputs are healthy -- lane 63 of wave 1, whose
    NaN the forecast does not read, included -- has the bits of the clean twin
    in the state, the stored precision, the status, the output rasters and H0;
    wave 3 takes the full path in A and the shortcut in B."""
    cp = problem(n_train)
    a, b = (launched(n_train, dev.type, key) for key in "AB")
    contained(a, b, launched(n_train, dev.type, "B", None, False), cp)
    assert np.isfinite(b["x"]).all() and np.isfinite(b["a"]).all() and np.isfinite(b["unc"]).all()
    assert not (b["status"] & K.ST_FALLBACK).any()


@pytest.mark.parametrize("n_train", N_TRAIN)
def test_status_equals_the_float64_classifier(dev, n_train):
    for key in "AB":
        got = launched(n_train, dev.type, key)["status"]
        want = model(n_train, key, dev.type == "cpu")["status"]
        assert np.array_equal(got, want), [(int(p), int(got[p]), int(want[p])) for p in np.nonzero(got != want)[0]]
    st = launched(n_train, dev.type, "A")["status"]
    dead = K.ST_BAD_OP | K.ST_NO_OBS | K.ST_NONFINITE | K.ST_FALLBACK | K.ST_OUT_OF_DOMAIN
    assert st[px(1, 3)] == dead and st[px(1, 33)] == dead
    assert st[px(1, 9)] == BAD and st[px(6, 26)] == BAD
    assert (st[px(1, 17)] & BAD) == BAD
    assert st[px(1, 63)] == 0
    assert st[px(1, 40)] == K.ST_NO_OBS
    assert (st[px(2, 0):px(3, 0)] == K.ST_NO_OBS).all()
    assert st[px(3, 35)] == BAD | K.ST_NO_OBS
    assert (np.delete(st[px(3, 0):px(4, 0)], 35) == K.ST_NO_OBS).all()
    # outside the line table is outside the emulators' training box, and nothing else
    assert st[px(4, 5)] == st[px(4, 44)] == K.ST_OUT_OF_DOMAIN
    assert st[px(5, 37)] == st[px(5, 58)] == K.ST_OUT_OF_DOMAIN | K.ST_NO_OBS


@pytest.mark.parametrize("n_train", N_TRAIN)
def test_nan_state_alone_declines_the_unobserved_wave_shortcut(dev, n_train):
    """Run C: the clean twin with a NaN in the propagated parameter of one lane
    of the unobserved wave 2 -- precision healthy, so only the shortcut's test
    of the linearisation point sends the wave down the full path, where the
    lane falls back and its 63 neighbours end on the shortcut's bits."""
    cp = problem(n_train)
    c, b = launched(n_train, dev.type, "C"), launched(n_train, dev.type, "B")
    p = px(2, 20)
    others = np.ones(cp["N"], bool)
    others[p] = False
    same_bits(c, b, others, OUT)
    want = model(n_train, "C", dev.type == "cpu")
    assert np.array_equal(c["status"], want["status"]), (int(c["status"][p]), int(want["status"][p]))
    assert c["status"][p] == K.ST_NO_OBS | K.ST_NONFINITE | K.ST_FALLBACK | K.ST_OUT_OF_DOMAIN
    assert (np.delete(c["status"][px(2, 0):px(3, 0)], 20) == K.ST_NO_OBS).all()
    assert np.array_equal(bits(c["x"][:, p]), bits(want["xf"][p]))
    # the lane counts 0, every other pixel what it counts in B (the host's sum order varies: test_norm_stays_finite)
    slack = 1e-13 * b["norm"] if dev.type == "cpu" else 0.0
    assert np.isfinite(c["norm"]) and abs(c["norm"] - b["norm"]) <= slack, (c["norm"], b["norm"])


@pytest.mark.parametrize("n_train", N_TRAIN)
def test_fallback_pixels_keep_the_forecast(dev, n_train):
    """x_out = the forecast mean bit for bit, the stored rows the forecast's,
    the uncertainty raster rsqrt of their diagonal (NaN where the diagonal is
    not positive: rsqrt of -1.04 has no finite value); nothing else
    non-finite outside the pixels whose inputs hold a NaN or an inf."""
    cp = problem(n_train)
    a = launched(n_train, dev.type, "A")
    m = model(n_train, "A", dev.type == "cpu")
    fb = np.nonzero(a["status"] & K.ST_FALLBACK)[0]
    assert set(fb) == {px(1, 3), px(1, 9), px(1, 17), px(1, 33), px(3, 35), px(6, 26)}
    assert np.array_equal(bits(a["x"][:, fb]), bits(m["xf"][fb].T))
    assert np.array_equal(bits(a["mean"][:, fb]), bits(a["x"][:, fb]))
    finite_fc = np.isfinite(m["xf"][fb]).all(1)
    assert np.isfinite(a["x"][:, fb[finite_fc]]).all() and list(fb[~finite_fc]) == [px(1, 3), px(1, 33)]
    # v_rcp_f32 / v_rsq_f32 and their host counterparts: 1 ulp each
    pf = pack_blocks(m["Pf"][fb])
    assert np.allclose(a["a"][:, fb], pf, rtol=1e-6, atol=0.0, equal_nan=True)
    d = np.einsum("nii->in", m["Pf"][fb])
    with np.errstate(invalid="ignore"):
        assert np.allclose(a["unc"][:, fb], 1.0 / np.sqrt(d), rtol=1e-6, atol=0.0, equal_nan=True)
    nonfinite_in = np.zeros(cp["N"], bool)
    nonfinite_in[[px(1, 3), px(1, 17), px(1, 33)]] = True
    for f in ("x", "a", "mean"):
        assert np.isfinite(a[f][:, ~nonfinite_in]).all(), f
    neg = np.zeros_like(a["unc"], dtype=bool)
    neg[6, [px(1, 9), px(3, 35), px(6, 26)]] = True      # p_a = -I: a forecast precision diagonal of -1.04
    assert np.isfinite(a["unc"][:, ~nonfinite_in][~neg[:, ~nonfinite_in]]).all()
    assert np.isnan(a["unc"][neg]).all()


@pytest.mark.parametrize("n_train", N_TRAIN)
def test_norm_stays_finite(dev, n_train):
    """The date's norm: over the pixels with a finite forecast (run M: the two
    others masked by healthy unobserved pixels, which count exactly 0) it is the
    oracle's sum over the pixels that keep their analysis; with the two pixels
    back in (run A) it is the same number, not NaN."""
    want = model(n_train, "M", dev.type == "cpu")["norm"]
    # without line tables every wave of both runs takes the GP sums: every pixel the two share has the same bits
    a, mk = launched(n_train, dev.type, "A", None, False), launched(n_train, dev.type, "M", None, False)
    al = launched(n_train, dev.type, "A")
    print(f"norm on {dev.type}, n_train {n_train}: masked {mk['norm']!r} oracle {want!r} corrupted {a['norm']!r}, "
          f"with line tables {al['norm']!r}")
    assert np.isfinite(mk["norm"]) and abs(mk["norm"] - want) / want < 1e-2, (mk["norm"], want)
    # the same float32 terms: the device's fixed-order float64 sum is the same number; the host runner's
    # OpenMP reduction adds its 411 float64 terms in a different order every run (411 * 2^-53 < 1e-13)
    slack = 1e-13 * mk["norm"] if dev.type == "cpu" else 0.0
    assert np.isfinite(a["norm"]) and abs(a["norm"] - mk["norm"]) <= slack, (a["norm"], mk["norm"])
    assert np.isfinite(al["norm"]) and abs(al["norm"] - want) / want < 1e-2, (al["norm"], want)


@pytest.mark.gpu
@pytest.mark.parametrize("n_train", N_TRAIN)
def test_healthy_pixels_against_float64(cuda, n_train):
    """The pixels that keep their analysis against the float64 oracle at the
    matrix-core tolerances of test_gpu.py::test_analysis_device_vs_host_and_oracle,
    H0 of wave 4 (GP sums) and of wave 5's observed lanes (line table) against
    the float64 emulators, and the proof that the two come from different paths."""
    cp = problem(n_train)
    a, h = launched(n_train, "cuda", "A"), launched(n_train, "cpu", "A")
    m = model(n_train, "A", False)
    keep = ~m["fallback"]
    xr, Ar = m["x"][keep], m["A"][keep]
    ex = float(np.max(np.abs(a["x"].T[keep] - xr) / (np.abs(xr) + 0.05)))
    d = np.sqrt(np.einsum("nii->ni", Ar))
    norm = d[:, :, None] * d[:, None, :]
    err_m = float(np.max(np.abs(unpack_blocks(a["a"], 7)[keep] - Ar) / norm))
    err_h = float(np.max(np.abs(unpack_blocks(h["a"], 7)[keep] - Ar) / norm))
    print(f"n_train {n_train}: x {ex:.2e}, A matrix cores {err_m:.2e} host {err_h:.2e}")
    assert ex < 2e-3, ex
    assert err_m < max(2e-4, 1.5 * err_h), (err_m, err_h)
    nl = launched(n_train, "cuda", "A", None, False)
    w4, w5 = slice(px(4, 0), px(5, 0)), slice(px(5, 0), px(5, 32))
    for b in range(2):
        obs = cp["A"]["prob"]["bands"][b][1] > 0
        e4 = float(np.abs(a["h0"][b][w4] - m["H"][b][w4])[obs[w4]].max())
        e5 = float(np.abs(a["h0"][b][w5] - m["H"][b][w5])[obs[w5]].max())
        print(f"band {b}: H0 wave 4 (GP sums) {e4:.2e}, wave 5 (line table) {e5:.2e}")
        assert e4 < 5e-6 and e5 < 2e-6, (b, e4, e5)
        assert obs[w4].any() and obs[w5].any()
        # without line tables wave 5 changes in the last bits and wave 4 not at all
        assert np.array_equal(bits(a["h0"][b][w4]), bits(nl["h0"][b][w4]))
        assert not np.array_equal(bits(a["h0"][b][w5]), bits(nl["h0"][b][w5]))
        assert float(np.abs(a["h0"][b][w5] - nl["h0"][b][w5]).max()) < 4e-6
    assert np.array_equal(a["status"], nl["status"])


@pytest.mark.gpu
@pytest.mark.parametrize("n_train", N_TRAIN)
def test_dense_and_generic_launches_agree_on_the_corrupted_run(cuda, n_train):
    """The forced-dense variant (line tables on) and the generic launch (off)
    on run A: the status bytes and every bit the clean runs of
    test_gpu_tip_structure.py agree on."""
    every = np.ones(problem(n_train)["N"], bool)
    for variant, line in ((K.Variant.DENSE_SOLVE, None), (K.Variant.GENERIC_SPEC, False)):
        got = launched(n_train, "cuda", "A", None, line)
        ref = launched(n_train, "cuda", "A", variant, line)
        assert ref["launches"]["tip"] == 0, ref["launches"]
        assert np.array_equal(got["status"], ref["status"])
        for f in ("x", "a", "mean", "unc"):
            assert np.array_equal(got[f], ref[f], equal_nan=True), (variant, f)
        same_bits(got, ref, every & ~problem(n_train)["corrupt"], ("x", "a", "mean", "unc"))
        assert got["norm"] == ref["norm"]


# ------------------------------------------------------------ spatial twin
def test_spatial_twin_decouples_the_sick_pixels(dev):
    """The regulariser's prepare (SPEC_PROP_REG_TIP on the device) over a raster
    64 wide, waves = rows: lanes 9 (p_a = -I) and 17 (NaN in p_a) of row 1 get
    V = 0 and u = x_f, nothing non-finite reaches u, V or the stored precision of
    another pixel, and every other pixel has the clean twin's bits."""
    cp = problem(160, True)
    N = cp["N"]
    geo = {"w": 64, "h": N // 64, "halo": 0, "n_up": 0}
    gamma = 2.0
    a, b = (C.containment_launch(cp[key], dev, reg=dict(gamma=gamma, mask=1 << 6, geo=geo)) for key in "AB")
    if dev.type == "cuda":
        assert a["launches"] == {"tip": 1, "dense": 0}, a["launches"]
    sick = np.array([px(1, 9), px(1, 17)])
    ok = ~cp["corrupt"]
    assert list(np.nonzero(~ok)[0]) == list(sick)
    same_bits(a, b, ok, ("x", "a", "status", "unc", "v", "h0"))
    rows, cols = np.divmod(np.arange(N), 64)
    deg = (rows > 0).astype(float) + (rows < N // 64 - 1) + (cols > 0) + (cols < 63)
    m = C.containment_model(cp["A"], dom=a["dom"], reg_gd=gamma * deg)
    assert np.array_equal(a["status"], m["status"]), np.nonzero(a["status"] != m["status"])[0]
    assert ((a["status"][sick] & BAD) == BAD).all() and not (a["status"][ok] & K.ST_FALLBACK).any()
    assert (a["v"][:, sick] == 0).all()
    assert np.array_equal(bits(a["x"][:, sick]), bits(m["xf"][sick].T))
    assert np.isfinite(a["x"]).all() and np.isfinite(a["v"]).all()
    assert np.isfinite(a["a"][:, ok]).all() and np.isfinite(a["unc"][:, ok]).all()
    ex = float(np.max(np.abs(a["x"].T[ok] - m["x"][ok]) / (np.abs(m["x"][ok]) + 0.05)))
    assert ex < 2e-3, ex


# ------------------------------------- 10-parameter global-table kernels
N10 = 2 * 64 + 19


@functools.lru_cache(maxsize=None)
def prosail10():
    """The PROSAIL problem of tests/test_gpu_gain_global.py; in the corrupted
    twin lane 5 of wave 0 has a NaN and lane 37 an inf in the linearisation
    point, which enter the exponent operand every lane of the wave shares."""
    prob = prosail_problem(N=N10, n_bands=10, seed=47, n_train=70)
    prob["x"] = prob["x"].astype(np.float32).astype(np.float64)
    bad = dict(prob, x=prob["x"].copy())
    bad["x"][5, 3] = np.nan
    bad["x"][37, 7] = np.inf
    return prob, bad


def _evals10(prob):
    with np.errstate(all="ignore"):
        return [em.predict(prob["x"]) + yw for em, yw in zip(prob["ems"], prob["bands"])]


@pytest.mark.gpu
def test_shared_operand_analysis_contains_nan_and_inf(cuda):
    """analysis_mfma_g_kernel<10, 10> with the exponent operand built once per
    iteration from every lane's x0 (BAND_LAYOUT_SHARED_X)."""
    clean, bad = prosail10()
    n, N = 10, N10
    res = []
    for prob in (bad, clean):
        tab = build_table(prob["specs"], dbands(prob, cuda), n, RecordCache(), cuda)
        assert tab.gpm_global and tab.gpm_frags == 0 and tab.layout == K.BAND_LAYOUT_SHARED_X
        xo = torch.zeros((n, N), device=cuda)
        ao = torch.zeros((ntri(n), N), device=cuda)
        st = torch.zeros(N, dtype=torch.uint8, device=cuda)
        part = K.partials_buffer(N, cuda)
        K.analysis(n, tab, C.soa(prob["x"], cuda), C.soa(prob["xf"], cuda), C.packed(prob["Pf"], cuda), xo, ao,
                   None, st, part)
        torch.cuda.synchronize()
        res.append(dict(x=xo.cpu().numpy(), a=ao.cpu().numpy(), status=st.cpu().numpy(), dom=tab.dom,
                        norm=float(K.reduce_partials(part).cpu())))
    a, b = res
    ok = np.ones(N, bool)
    ok[[5, 37]] = False
    same_bits(a, b, ok, ("x", "a", "status"))
    xf32 = clean["xf"].astype(np.float32).astype(np.float64)
    pf32 = clean["Pf"].astype(np.float32).astype(np.float64)
    m = C.info_model(bad["x"], xf32, pf32, _evals10(bad), dom=a["dom"])
    assert np.array_equal(a["status"], m["status"]), [(int(p), int(a["status"][p]), int(m["status"][p]))
                                                      for p in np.nonzero(a["status"] != m["status"])[0]]
    dead = K.ST_BAD_OP | K.ST_NO_OBS | K.ST_NONFINITE | K.ST_FALLBACK
    assert ((a["status"][[5, 37]] & dead) == dead).all() and not (a["status"][ok] & K.ST_FALLBACK).any()
    # the fallback keeps the (finite) forecast, and the norm is finite
    assert np.array_equal(bits(a["x"][:, [5, 37]]), bits(clean["xf"][[5, 37]].T))
    assert np.isfinite(a["x"]).all() and np.isfinite(a["a"]).all() and np.isfinite(a["norm"])
    keep = ~m["fallback"]
    assert x_err(a["x"].T[keep], m["x"][keep]) < 2e-3


def _gain_status(xf, cov, bands_w, evals):
    """The gain form's status byte: ST_NONSPD where the Cholesky factorisation of
    the analysis covariance fails (gain_forecast), ST_BAD_OP / ST_NO_OBS as the
    information form, ST_NONFINITE | ST_FALLBACK where the state is not finite
    (the factorisation replaces a failed pivot, so nothing else becomes
    non-finite)."""
    N = xf.shape[0]
    st = np.zeros(N, np.uint8)
    if cov is not None:
        spd, _ = C.chol_model(cov, np.zeros(xf.shape))
        st[~spd] |= K.ST_NONSPD
    nobs = np.zeros(N, int)
    for (H, h), w in zip(evals, bands_w):
        ok = np.isfinite(H) & np.isfinite(h).all(1)
        st[(w > 0) & ~ok] |= K.ST_BAD_OP
        nobs += (w > 0) & ok
    st[nobs == 0] |= K.ST_NO_OBS
    st[~np.isfinite(xf).all(1)] |= K.ST_NONFINITE | K.ST_FALLBACK
    return st


@pytest.mark.gpu
def test_gain_global_kernel_contains_nan_and_inf(cuda):
    """gain_mfma_g_kernel<10, 10>, the same corrupted lanes: their operators
    are ST_BAD_OP, so no band updates them and they end on the forecast."""
    clean, bad = prosail10()
    n, N = 10, N10
    cov = np.linalg.inv(clean["Pf"])
    res = []
    for prob in (bad, clean):
        tab = build_table(prob["specs"], dbands(prob, cuda), n, RecordCache(), cuda)
        assert tab.gpm_global and tab.layout == K.BAND_LAYOUT_SHARED_X
        xo = torch.zeros((n, N), device=cuda)
        po = torch.zeros((ntri(n), N), device=cuda)
        st = torch.zeros(N, dtype=torch.uint8, device=cuda)
        part = K.partials_buffer(N, cuda)
        K.gain(n, tab, C.soa(prob["x"], cuda), C.soa(prob["xf"], cuda), C.packed(cov, cuda), xo, po, st, part)
        torch.cuda.synchronize()
        res.append(dict(x=xo.cpu().numpy(), a=po.cpu().numpy(), status=st.cpu().numpy(),
                        norm=float(K.reduce_partials(part).cpu())))
    a, b = res
    ok = np.ones(N, bool)
    ok[[5, 37]] = False
    same_bits(a, b, ok, ("x", "a", "status"))
    ev = _evals10(bad)
    want = _gain_status(clean["xf"], None, [e[3] for e in ev], [e[:2] for e in ev])
    assert np.array_equal(a["status"], want), np.nonzero(a["status"] != want)[0]
    assert (a["status"][[5, 37]] == K.ST_BAD_OP | K.ST_NO_OBS).all()
    assert np.array_equal(bits(a["x"][:, [5, 37]]), bits(clean["xf"][[5, 37]].T))
    assert np.isfinite(a["x"]).all() and np.isfinite(a["a"]).all()
    xr, Pr = gain_blocks(clean["x"][ok], clean["xf"][ok], cov[ok], [tuple(v[ok] for v in e) for e in _evals10(clean)])
    ex = x_err(a["x"].T[ok], xr)
    d = np.sqrt(np.einsum("nii->ni", Pr))
    ep = float(np.max(np.abs(unpack_blocks(a["a"], n)[ok] - Pr) / (d[:, :, None] * d[:, None, :])))
    print(f"gain <10, 10>: x {ex:.2e} P {ep:.2e}")
    assert ex < 1e-4 and ep < 2e-4, (ex, ep)


@pytest.mark.gpu
@pytest.mark.parametrize("n_train", N_TRAIN)
def test_gain_tip_kernel_contains_the_corrupted_lanes(cuda, n_train):
    """gain_mfma_kernel (JRC-TIP, LDS tables) over the containment runs with the
    forecast fused from the analysis covariance: the -I and NaN blocks are
    ST_NONSPD (gain_forecast), the NaN / inf states ST_NONFINITE | ST_FALLBACK."""
    cp = problem(n_train)
    n, N = 7, cp["N"]
    cov_b = np.linalg.inv(cp["B"]["pa"])
    cov_a = cov_b.copy()
    for p in (px(1, 9), px(3, 35), px(6, 26)):
        cov_a[p] = -np.eye(n)
    cov_a[px(1, 17), 6, 6] = np.nan
    res = []
    for key, cov, line in (("A", cov_a, None), ("B", cov_b, None), ("B", cov_b, False)):
        run = cp[key]
        h0 = [torch.zeros(N, dtype=torch.float32, device=cuda) for _ in range(2)]
        tab = C.table(run["prob"], cuda, h0_outs=h0)
        assert tab.gpm_frags > 0
        xo = torch.zeros((n, N), device=cuda)
        po = torch.zeros((ntri(n), N), device=cuda)
        mean = torch.zeros((n, N), device=cuda)
        unc = torch.zeros((n, N), device=cuda)
        st = torch.zeros(N, dtype=torch.uint8, device=cuda)
        part = K.partials_buffer(N, cuda)
        h = K.prop_args(n, C.containment_spec(n), C.soa(run["xa"], cuda), C.packed(cov, cuda), fused=True)
        K.gain(n, tab, None, None, None, xo, po, st, part, prop=h, out=(mean, unc, None), line=line)
        torch.cuda.synchronize()
        res.append(dict(x=xo.cpu().numpy(), a=po.cpu().numpy(), status=st.cpu().numpy(), mean=mean.cpu().numpy(),
                        unc=unc.cpu().numpy(), h0=[t.cpu().numpy() for t in h0],
                        norm=float(K.reduce_partials(part).cpu())))
    a, b, b_sums = res
    contained(a, b, b_sums, cp)
    m = model(n_train, "A", False)
    xf = m["xf"]
    with np.errstate(all="ignore"):
        ev = [cp["A"]["prob"]["ems"][bi].predict(xf[:, k.TIP_BAND_MAPPER[bi]]) for bi in range(2)]
    want = _gain_status(xf, cov_a.astype(np.float32).astype(np.float64),
                        [yw[1] for yw in cp["A"]["prob"]["bands"]], ev)
    assert np.array_equal(a["status"], want), [(int(p), int(a["status"][p]), int(want[p]))
                                               for p in np.nonzero(a["status"] != want)[0]]
    dead = K.ST_BAD_OP | K.ST_NO_OBS | K.ST_NONFINITE | K.ST_FALLBACK
    assert a["status"][px(1, 3)] == dead and a["status"][px(1, 33)] == dead
    assert a["status"][px(1, 9)] == a["status"][px(1, 17)] == a["status"][px(6, 26)] == K.ST_NONSPD
    assert a["status"][px(3, 35)] == K.ST_NONSPD | K.ST_NO_OBS and a["status"][px(1, 40)] == K.ST_NO_OBS
    assert np.isfinite(a["norm"]), a["norm"]
    # healthy pixels against gain_blocks over the float64 forecast covariance
    ok = ~cp["corrupt"]
    Pi = k.tip_prior()[2]
    Cf = np.broadcast_to(Pi, (N, n, n)).copy()
    Cf[:, 6, 6] = 1.0 / (1.0 / np.linalg.inv(cov_b)[:, 6, 6] + C.CONTAIN_Q)
    Pf = np.linalg.inv(Cf)
    bands = [(ev[bi][0], np.zeros((N, n)), *cp["A"]["prob"]["bands"][bi]) for bi in range(2)]
    for bi in range(2):
        bands[bi][1][:, k.TIP_BAND_MAPPER[bi]] = ev[bi][1]
    xr, Pr = gain_blocks(xf[ok], xf[ok], Pf[ok], [tuple(v[ok] for v in bd) for bd in bands])
    ex = x_err(a["x"].T[ok], xr)
    d = np.sqrt(np.einsum("nii->ni", Pr))
    ep = float(np.max(np.abs(unpack_blocks(a["a"], n)[ok] - Pr) / (d[:, :, None] * d[:, None, :])))
    print(f"gain TIP, n_train {n_train}: x {ex:.2e} P {ep:.2e}")
    assert ex < 1e-4 and ep < 2e-4, (ex, ep)
