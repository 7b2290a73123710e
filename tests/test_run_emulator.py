"""run_emulator (reference utils.py:68-106): host NumPy path vs the resident
tensor path (torch.unique + K7 LUT assignment on the tensor's device)."""
import numpy as np
import pytest
import torch

from kafka_inferenceengine_amd.models.gp import GaussianProcessEmulator
from kafka_inferenceengine_amd.models.operators import locate_in_lut, run_emulator

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]


def _gp(D=4, T=40, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (T, D))
    y = np.sin(X @ rng.normal(size=D))
    return GaussianProcessEmulator.fit(X, y, lengthscale=np.full(D, 0.5), noise=1e-3)


@pytest.mark.parametrize("device", DEVICES)
def test_run_emulator_unique_rows_device_equals_host(device):
    gp = _gp()
    rng = np.random.default_rng(1)
    base = rng.uniform(0, 1, (50, 4)).astype(np.float32)
    x = base[rng.integers(0, 50, 3000)]              # 3000 rows, 50 unique
    H, dH = run_emulator(gp, x.astype(np.float64))
    Ht, dHt = run_emulator(gp, torch.as_tensor(x, device=device))
    assert Ht.device.type == device and Ht.shape == (3000,) and dHt.shape == (3000, 4)
    np.testing.assert_allclose(Ht.cpu().numpy(), H, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(dHt.cpu().numpy(), dH, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("device", DEVICES)
def test_run_emulator_lut_branch_device_equals_host(device):
    gp = _gp()
    rng = np.random.default_rng(2)
    x = rng.normal(0.5, 0.1, (4000, 4)).astype(np.float32)
    H, dH = run_emulator(gp, x.astype(np.float64), lut_threshold=100, lut_size=300, seed=7)
    Ht, dHt = run_emulator(gp, torch.as_tensor(x, device=device), lut_threshold=100,
                           lut_size=300, seed=7)
    lut = np.random.default_rng(7).multivariate_normal(
        x.astype(np.float64).mean(0), np.cov(x.astype(np.float64), rowvar=False), 300)
    near = locate_in_lut(lut, x)
    # every pixel takes its nearest LUT row's emulator value; ties between
    # f32 (device) and f64 (host) distances are the only allowed difference
    same = np.isclose(Ht.cpu().numpy(), H, rtol=1e-4, atol=1e-5)
    assert same.mean() > 0.995
    pred = np.asarray(gp.predict(lut, do_unc=False)[0])
    np.testing.assert_allclose(H, pred[near], rtol=1e-12)
    assert dHt.shape == (4000, 4) and np.isfinite(dHt.cpu().numpy()).all()


@pytest.mark.parametrize("D", [4, 7, 10])
@pytest.mark.parametrize("device", DEVICES)
def test_run_emulator_default_lut_size_device_equals_host(device, D, monkeypatch):
    """The LUT branch at the reference's own LUT size (the default, 5000 rows;
    200,000 bytes of float32 for a full PROSAIL state) on 4096 + 37 rows.  The
    K7 assignment the tensor path makes is held to float64 over the float32 LUT
    and points it was given: every pixel's chosen row within (1 + 1e-5) of the
    smallest squared distance, the float64 argmin on at least 99.9 % of the
    pixels; the tensor path returns that row's emulator value, which is the
    host NumPy path's on at least 99.9 % of the pixels (float32 against float64
    distances may resolve a near tie differently)."""
    from kafka_inferenceengine_amd.ops import kernels as K

    gp = _gp(D=D)
    rng = np.random.default_rng(10 + D)
    G = rng.normal(size=(D, D))
    x = rng.multivariate_normal(np.full(D, 0.5), 0.01 * (G @ G.T / D + 0.5 * np.eye(D)), 4096 + 37).astype(np.float32)
    seen = {}
    k7 = K.lut_nearest

    def recording(lut, pts, *a, **kw):
        out = k7(lut, pts, *a, **kw)
        seen.update(lut=lut.cpu().numpy().astype(np.float64), pts=pts.cpu().numpy().astype(np.float64).T,
                    idx=out.cpu().numpy().astype(np.int64))
        return out

    monkeypatch.setattr(K, "lut_nearest", recording)
    H, dH = run_emulator(gp, x.astype(np.float64), lut_threshold=100, seed=7)
    Ht, dHt = run_emulator(gp, torch.as_tensor(x, device=device), lut_threshold=100, seed=7)
    assert seen["lut"].shape == (5000, D) and seen["idx"].shape == (len(x),)
    lut, pts, idx = seen["lut"], seen["pts"], seen["idx"]
    near = np.empty(len(pts), np.int64)
    for s in range(0, len(pts), 512):
        near[s:s + 512] = ((lut * lut).sum(1)[None, :] - 2.0 * pts[s:s + 512] @ lut.T).argmin(1)
    dist = lambda j: ((lut[j] - pts) ** 2).sum(1)  # noqa: E731
    assert idx.min() >= 0 and idx.max() < 5000
    assert np.all(dist(idx) <= (1.0 + 1e-5) * dist(near))
    assert (idx == near).mean() >= 0.999
    pred, dpred = gp.predict(lut, do_unc=False)
    assert Ht.device.type == device and Ht.shape == (len(x),) and dHt.shape == (len(x), D)
    np.testing.assert_allclose(Ht.cpu().numpy(), pred[idx], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(dHt.cpu().numpy(), dpred[idx], rtol=1e-5, atol=1e-5)
    same = np.isclose(Ht.cpu().numpy(), H, rtol=1e-4, atol=1e-5)
    assert same.mean() >= 0.999, same.mean()


@pytest.mark.parametrize("device", DEVICES)
def test_run_emulator_float64_rows_that_collide_in_float32(device):
    """float64 rows that differ only below float32 precision stay
    distinct on the tensor path (deduplicated in the input's precision, as on
    the host path), and the results come back in float64."""
    gp = _gp()
    rng = np.random.default_rng(4)
    base = rng.uniform(0.2, 0.8, (20, 4))
    x = np.repeat(base, 3, axis=0)
    x[1::3, 0] += 1e-11          # same float32 row, a different float64 row
    x[2::3, 2] -= 3e-12
    assert len(np.unique(x.astype(np.float32), axis=0)) == 20 and len(np.unique(x, axis=0)) == 60
    H, dH = run_emulator(gp, x)
    Ht, dHt = run_emulator(gp, torch.as_tensor(x, device=device))
    assert Ht.dtype == torch.float64 and dHt.dtype == torch.float64
    np.testing.assert_allclose(Ht.cpu().numpy(), H, rtol=1e-13, atol=1e-14)
    np.testing.assert_allclose(dHt.cpu().numpy(), dH, rtol=1e-12, atol=1e-13)
