"""``K.gp_operator(gp="f64")`` (csrc/kf_gp_operator_f64.hip) against the float64 emulator's ``predict``.  Per observed
pixel the error is bounded by one float32 rounding of the result (a half ulp, a factor 2 allowed: 2^-23) plus 2^-36 of
the term scale: (D + 2) roundings of 2^-53 on exponent terms up to 2^10, T float64 roundings in the sums and the
exponential's 2^-45 come to about 2^-39 of it, and 2^-36 leaves 8x over that."""
import dataclasses
import datetime as dt

import numpy as np
import pytest
import torch

import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.ops import kernels as K

import gp_operator_cases as G
import kernel_cases as C
from test_gpu_aux import pad_untouched

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
# (n, maps): D = 1, 2, 4 through the JRC-TIP maps, 5 (NK = 2 with three padded slots), 7, 10, and 7 + 4 in one call
SHAPES = {"d1": (2, ((0,), (1,))), "d2": (3, ((0, 2), (1, 0))), "d4 tip": (7, tuple(tuple(k.TIP_BAND_MAPPER[b]) for b in (0, 1))),
          "d5": (7, ((0, 2, 4, 6, 1), (6, 5, 4, 3, 2))), "d7": (7, (tuple(range(7)),) * 2),
          "d10": (10, (tuple(range(10)),) * 2), "mixed": (7, G.MAPS_7_MIXED)}


def launch(n, tab, x0, N, pad):
    ldh = N + pad + 3
    h0, h = C.sentinel(2, ldh, DEV), C.sentinel(2 * n, ldh, DEV)
    K.gp_operator(n, tab, C.padded(x0.T, N + pad, DEV, fill=-777.0), h0, h, N=N, gp="f64")
    assert K.LAST_GP_OPERATOR_PLAN["family"] == K.GP_OPERATOR_F64_KERNEL
    assert pad_untouched(h0, N) and pad_untouched(h, N), (N, pad)
    return h0[:, :N].cpu().numpy(), h[:, :N].cpu().numpy()


def errors(tag, evals, maps, T, x0, n, h0, h):
    """Worst error / bound (value, gradient) over the observed pixels, the term scales from the emulator's own X,
    alpha and lam in float64; masked pixels hold +0.0 in h0 and all n rows, unmapped state rows exactly 0."""
    worst = [0.0, 0.0]
    for b, (H, hr, _, w) in enumerate(evals):
        on, mp, em = w > 0, list(maps[b]), G.emulator(len(maps[b]), T[b])
        g = np.column_stack([h0[b], h[b * n:(b + 1) * n].T]).astype(np.float64)
        assert len(w) < 63 or (~on).any(), "the case must mask some pixels"
        assert not g[~on].any() and not np.signbit(g[~on]).any(), (tag, b)
        diff = x0[on][:, mp][:, None, :] - em.inputs[None]
        ak = np.abs(em.alpha * em.signal * np.exp(-0.5 * np.einsum("ntd,d->nt", diff * diff, em.lam)))
        bound = np.zeros((int(on.sum()), 1 + n))
        bound[:, 0] = 2.0 ** -23 * np.abs(H[on]) + 2.0 ** -36 * ak.sum(1)
        bound[:, 1 + np.array(mp)] = 2.0 ** -23 * np.abs(hr[on][:, mp]) + \
            2.0 ** -36 * np.einsum("nt,ntd->nd", ak, np.abs(em.lam * diff))
        err = np.abs(g[on] - np.column_stack([H[on], hr[on]]))
        assert not err[bound == 0].any(), (tag, b)
        ratio = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)
        worst = [max(worst[0], ratio[:, 0].max(initial=0.0)), max(worst[1], ratio[:, 1:].max(initial=0.0))]
    print(f"MEASURE gp_operator f64 {tag}: worst error / bound value {worst[0]:.3f} gradient {worst[1]:.3f}")
    return worst


@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_vs_float64(shape):
    n, maps = SHAPES[shape]
    worst = [0.0, 0.0]
    for i in range(len(C.AUX_N)):
        N, pad = C.aux_shape(list(SHAPES).index(shape) + i)
        x0, evals, table = G.case(n, maps, N)
        h0, h = launch(n, table(DEV, pad), x0, N, pad)
        assert len(K.LAST_GP_OPERATOR_PLAN["names"]) == (2 if shape == "mixed" else 1)
        worst = np.maximum(worst, errors(f"{shape} N={N}", evals, maps, (64, 64), x0, n, h0, h))
    assert worst[0] <= 1.0 and worst[1] <= 1.0, worst


@pytest.mark.parametrize("n,T,what", [(4, (17, 16), "T = 17 and 16"), (4, (513, 64), "T = 513"),
                                      (7, (64, 64), "three pixel groups"), (7, (64, 64), "dark wave")])
def test_table_sizes_and_a_masked_wave(n, T, what):
    """T = 17 (two groups, 15 padded points) beside T = 16, T = 513, one workgroup per band walking three pixel
    groups, and a 64-pixel tile no lane of which observes the band."""
    N, pad, maps = 257 + 256, 5, (tuple(range(n)),) * 2
    x0, evals, table = G.case(n, maps, N, T=T, dark=slice(64, 128) if what == "dark wave" else None)
    K.ext().set_max_blocks(2 if what == "three pixel groups" else 0)   # 2: one workgroup per band
    try:
        h0, h = launch(n, table(DEV, pad), x0, N, pad)
    finally:
        K.ext().set_max_blocks(0)
    assert max(errors(what, evals, maps, T, x0, n, h0, h)) <= 1.0


def test_nan_input_poisons_its_own_pixel_only():
    n, N, pad = 7, 257 + 256, 64
    x0, evals, table = G.case(n, G.MAPS_7_MIXED, N)
    px = int(np.flatnonzero((evals[0][3][130:] > 0) & (evals[1][3][130:] > 0))[0]) + 130   # observed in both bands
    tab = table(DEV, pad)
    clean = launch(n, tab, x0, N, pad)
    x0[px, 0] = np.nan                       # state 0 feeds both bands
    bad = launch(n, tab, x0, N, pad)
    for a, b in zip(clean, bad):
        assert np.array_equal(np.delete(a, px, 1), np.delete(b, px, 1)) and np.isnan(b[:, px]).any()


def test_refusals_leave_the_valu_call_working():
    """CPU tensors, a linear band and specs without an emulator (records only): ValueError with gp="f64"; the same
    call with gp="valu" runs (the linear band's on the host runner: the device's VALU kernels are GP-only)."""
    n, N, cpu = 4, 65, torch.device("cpu")
    x0, _, table = G.case(n, (range(n),) * 2, N)
    lin = C.nongp_case(n, N, (("gp", K.OBS_F32), ("linear", K.OBS_F32)))

    def records_only(dev):
        tab = table(dev, 0)
        return dataclasses.replace(tab, specs=tuple(dataclasses.replace(s, emulator=None) for s in tab.specs))

    for dev, vdev, tab_of in ((cpu, cpu, lambda d: table(d, 0)), (DEV, cpu, lambda d: C.nongp_table(lin, d, 0)[0]),
                              (DEV, DEV, records_only)):
        with pytest.raises(ValueError, match="gp_operator\\(gp='f64'\\)"):
            K.gp_operator(n, tab_of(dev), C.padded(x0.T, N, dev), C.sentinel(2, N, dev), C.sentinel(2 * n, N, dev),
                          N=N, gp="f64")
        h0 = C.sentinel(2, N, vdev)
        K.gp_operator(n, tab_of(vdev), C.padded(x0.T, N, vdev), h0, C.sentinel(2 * n, N, vdev), N=N, d=n, gp="valu")
        assert torch.isfinite(h0).all() and bool((h0 != C.SENTINEL).all())


def test_engine_split_path_in_float64():
    """tests/test_gpu_gp_operator_mfma.py test_engine_split_path_on_the_matrix_cores' problem and tolerances, f64
    against valu."""
    mask = np.ones((10, 9), bool)
    obs = k.SyntheticS2Observations(mask, n_bands=10, n_train=30, device=DEV, stream=False, n_pool=2, field_cell=4)
    prior = k.SAILPrior(k.SAIL_PARAMETERS, mask)
    x0, Pinv = prior.process_prior(None)
    grid = [obs.dates[0] - dt.timedelta(days=1), obs.dates[1] + dt.timedelta(days=1)]
    res = []
    for gp in ("valu", "f64"):
        K.LAST_GP_OPERATOR_PLAN = None
        kf = k.LinearKalman(obs, None, mask, k.create_prosail_observation_operator, k.SAIL_PARAMETERS,
                            state_propagation=None, prior=prior, device=DEV,
                            config=k.EngineConfig(gp_split="always", split_gp=gp, band_chunk=3))
        res.append((kf.run(grid, x0, None, Pinv), [h["gn_iterations"] for h in kf.history]))
        assert (K.LAST_GP_OPERATOR_PLAN is not None) == (gp == "f64")
    assert K.LAST_GP_OPERATOR_PLAN["family"] == K.GP_OPERATOR_F64_KERNEL
    (a, ia), (b, ib) = res
    assert ia == ib and torch.allclose(a.x, b.x, rtol=1e-4, atol=1e-5)
    assert torch.allclose(a.P, b.P, rtol=1e-4, atol=1e-2)
