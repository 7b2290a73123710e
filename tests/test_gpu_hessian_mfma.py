"""K6 with the GP sums on the matrix cores (csrc/kf_gp_mfma.h pixel_hessian_mfma,
``K.hessian(gp="mfma")``) on the device against float64
``a0 - sum_b w (y - predict) hessian``, beside the VALU kernel on the same cases.

Bounds: the project's K6 bound, 2e-3 of the largest entry of the correction
(tests/test_gpu_aux.py), and at most 4x the VALU kernel's worst error over the
N of a layout: split-f16 operands keep 22 significant bits, float32 24.  N walks
below a wave, around one and five tiles with a tail; the leading dimension is
N + 5 with a sentinel in the padding.

The float64 comparison is parametrised over the layout and n_train and walks
the N inside one test, since the 4x bound is on the worst error over them.

Measured worst error over N, of the largest entry of the correction (MI355X):
    layout   n_train  VALU     matrix cores
    tip      24       3.0e-6   7.5e-6
    tip      40       1.4e-4   5.5e-5
    tip      70       3.1e-5   4.4e-5
    prosail  24       2.4e-6   3.2e-6
    prosail  40       4.8e-6   2.5e-6
    prosail  70       2.9e-6   2.8e-6
"""
import datetime as dt
import functools

import numpy as np
import pytest
import torch

import kafka_inferenceengine_amd as k
import kernel_cases as C
from kafka_inferenceengine_amd.engine.bands import DeviceBand, RecordCache, build_table
from kafka_inferenceengine_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
LAYOUTS = ("tip", "prosail")
NTRAIN = (24, 40, 70)          # one chunk, a padded second chunk, three chunks
NS = (1, 63, 64, 65, 64 * 5 + 3)
PAD = 5
BAD = 100                      # the pixel of the containment cases (N = 323: tile 1, used in every band)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


@functools.lru_cache(maxsize=None)
def _case(layout, n_train, N):
    """``kernel_cases.hessian_case`` with ``n_train`` a parameter: two JRC-TIP bands or three full-state
    PROSAIL bands.  A fifth of the pixels is masked in every band; for N > 64 the whole first tile is."""
    from kafka_inferenceengine_amd.utils.blocks import unpack_blocks
    rng = np.random.default_rng([n_train, N, LAYOUTS.index(layout)])
    if layout == "tip":
        n, ems, maps = 7, k.make_tip_emulators(n_train=n_train, seed=0), [list(m) for m in k.TIP_BAND_MAPPER[:2]]
        mu, P, _ = k.tip_prior()
        x = mu[None, :] + rng.normal(size=(N, 7)) * np.sqrt(np.diag(P)) * 0.3
        x[:, 6] = np.clip(x[:, 6], 0.05, 0.95)
    else:
        n, ems = 10, k.make_prosail_emulators(n_bands=3, n_train=n_train, seed=0)
        maps = [list(range(10))] * 3
        lo, hi = np.min([em.inputs.min(0) for em in ems], 0), np.max([em.inputs.max(0) for em in ems], 0)
        x = lo + (hi - lo) * (0.2 + 0.6 * rng.random((N, 10)))
    x = C.f32(x)
    masked = rng.random(N) < 0.2
    masked[0] = False
    if N > 64:
        masked[:64], masked[min(BAD, N - 1)] = True, False
    obs, corr = [], np.zeros((N, n, n))
    for em, mp in zip(ems, maps):
        f = em.predict(x[:, mp])[0]
        y, w = C.f32(f + 0.01 * rng.normal(size=N)), C.f32(np.where(masked, 0.0, 1.0 / 0.02 ** 2))
        obs.append((y, w))
        corr[np.ix_(np.arange(N), mp, mp)] += (w * (y - f))[:, None, None] * em.hessian(x[:, mp])
    a0 = C.f32(rng.normal(size=(n * (n + 1) // 2, N)))
    return dict(n=n, N=N, x=x, obs=obs, specs=[k.gp_spec(em, mp) for em, mp in zip(ems, maps)], masked=masked,
                a0=a0, corr=corr, ref=unpack_blocks(a0, n) - corr)


def _launch(c, dev, gp, x=None):
    n, N, ld = c["n"], c["N"], c["N"] + PAD
    db = [DeviceBand(K.OBS_F32, y=torch.from_numpy(y.astype(np.float32)).to(dev),
                     w=torch.from_numpy(w.astype(np.float32)).to(dev)) for y, w in c["obs"]]
    tab = build_table(c["specs"], db, n, RecordCache(), dev)
    a = C.padded(c["a0"], ld, dev)
    K.hessian(n, tab, C.padded((c["x"] if x is None else x).T, ld, dev), a, N=N, gp=gp)
    return a.cpu().numpy()


@pytest.mark.parametrize("n_train", NTRAIN)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_vs_float64_and_valu(dev, layout, n_train):
    from kafka_inferenceengine_amd.utils.blocks import unpack_blocks
    worst = {"valu": 0.0, "mfma": 0.0}
    for N in NS:
        c = _case(layout, n_train, N)
        scale = np.abs(c["corr"]).max()
        for gp in ("valu", "mfma"):
            a = _launch(c, dev, gp)
            assert np.all(a[:, N:] == C.SENTINEL)
            assert np.array_equal(a[:, :N][:, c["masked"]], c["a0"][:, c["masked"]])
            err = np.abs(unpack_blocks(a[:, :N], c["n"]) - c["ref"]).max() / scale
            print(f"hessian {gp} {layout} T={n_train} N={N}: {err:.2e} of the largest entry ({scale:.2e})")
            worst[gp] = max(worst[gp], err)
        assert K.LAST_HESSIAN_PLAN["family"] == "hessian_mfma_kernel"
    print(f"hessian {layout} T={n_train} worst: valu {worst['valu']:.2e} mfma {worst['mfma']:.2e}")
    assert worst["mfma"] < 2e-3
    assert worst["mfma"] <= 4 * worst["valu"]


@pytest.mark.parametrize("bad", [np.nan, 1e30])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_bad_pixel_stays_contained(dev, layout, bad):
    c = _case(layout, 40, NS[-1])
    clean = _launch(c, dev, "mfma")
    x = c["x"].copy()
    x[BAD] = bad
    got = _launch(c, dev, "mfma", x=x)
    others = np.arange(got.shape[1]) != BAD
    assert np.array_equal(got[:, others], clean[:, others], equal_nan=True)
    assert not np.array_equal(got[:, BAD], clean[:, BAD])


def _engine_date(dev, **cfg):
    mask = np.ones((16, 16), bool)
    obs = k.SyntheticBHRObservations(mask, n_train=80, stream=False, n_pool=5, device=dev, seed=0, field_cell=8)
    x0, Pinv = k.JRCPrior(k.TIP_PARAMETERS, mask).process_prior(None)
    kf = k.LinearKalman(obs, None, mask, k.create_nonlinear_observation_operator, k.TIP_PARAMETERS,
                        state_propagation=k.propagate_information_filter_LAI, device=dev, config=k.EngineConfig(**cfg))
    kf.set_trajectory_model()
    kf.set_trajectory_uncertainty(np.zeros_like(x0))
    st = kf.run([dt.datetime(2017, 1, 1), dt.datetime(2017, 1, 17)], x0, None, Pinv)
    return st.x.cpu().numpy(), st.P.cpu().numpy()


def test_engine_option(dev):
    x_off, p_off = _engine_date(dev, hessian_correction=False)
    K.LAST_HESSIAN_PLAN = None
    x_m, p_m = _engine_date(dev, hessian_correction=True, hessian_gp="mfma")
    assert K.LAST_HESSIAN_PLAN["name"] == "hessian_mfma_kernel<7, 4>"
    x_v, p_v = _engine_date(dev, hessian_correction=True, hessian_gp="valu")
    assert K.LAST_HESSIAN_PLAN["family"] == "pixel_kernel"
    corr = np.abs(p_v - p_off).max()
    assert corr > 0 and np.array_equal(x_m, x_v)
    assert np.abs(p_m - p_v).max() <= 2 * 2e-3 * corr


def test_unsupported_table_raises(dev):
    c = C.hessian_case(4, 65)
    db = [DeviceBand(K.OBS_F32, y=torch.from_numpy(y.astype(np.float32)).to(dev),
                     w=torch.from_numpy(w.astype(np.float32)).to(dev)) for y, w in c["obs"]]
    tab = build_table(c["specs"], db, 4, RecordCache(), dev)
    assert not K.hessian_mfma_supported(4, tab, dev)
    x, a = C.padded(c["x"].T, 70, dev), C.padded(c["a0"], 70, dev)
    with pytest.raises(ValueError, match="no matrix-core Hessian kernel"):
        K.hessian(4, tab, x, a, N=65, gp="mfma")
