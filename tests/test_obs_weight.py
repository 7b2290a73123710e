"""Observation weights inflated by the emulator's predictive variance (``K.gp_variance(obs=...)``,
csrc/kf_gp_variance.hip ``gp_obs_weight_kernel``) without a GPU: the host runner against float64, and
the ``emulator_uncertainty`` values.  ``band`` and ``check`` also serve test_gpu_obs_weight.py.

Reference: (y, w) from ``DeviceBand.decode()``, var from the float64 ``variance``, w_ref = 1 / (1/w + var).
Bound on |w' - w_ref| / w_ref: w_ref allow s + 6 2^-23 -- dw' = w'^2 dvar with the cases' allowance
(gp_variance_cases.py, in units of s) for dvar, and at most six roundings of 2^-23 (the decode's
reciprocal, square and product, the fma, the division, the store)."""
import numpy as np
import pytest
import torch

import gp_variance_cases as V
import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.engine.bands import DeviceBand
from kafka_inferenceengine_amd.ops import kernels as K

ENCODINGS = ("dn16", "f32mask", "bf16", "bf16y")
PAD, SENTINEL = 5, -7.0


def band(encoding, N, dev="cpu"):
    """Reflectances in (0.05, 0.5) with sigma = max(5 % y, 0.004), so w = 1.6e3 .. 6e4 against variances
    of 1e-5 .. 8e-3: w var > 0.1 on most pixels (asserted in ``check``).  About one pixel in seven is
    nodata and so is all of the tile 64..127 (N = 1: observed); the planes are PAD longer than N."""
    rng = np.random.default_rng([N, ENCODINGS.index(encoding)])
    y = np.zeros(N + PAD, np.float32)
    y[:N] = rng.uniform(0.05, 0.5, N)
    gone = np.ones(N + PAD, bool)
    gone[:N] = (rng.random(N) < 0.15) & (N > 1)
    gone[64:128] = True
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    bits = lambda a: t(a).to(torch.bfloat16).view(torch.int16)       # noqa: E731
    unc = dict(rel_unc=0.05, unc_floor=0.004)
    if encoding == "dn16":
        return DeviceBand(K.OBS_DN16, dn=t(np.where(gone, 0, np.rint(y / 1e-4)).astype(np.int16)), scale=1e-4, **unc)
    if encoding == "bf16y":
        return DeviceBand(K.OBS_BF16Y, y=bits(np.where(gone, np.nan, y).astype(np.float32)), **unc)
    w = (1.0 / np.maximum(0.05 * y, 0.004) ** 2).astype(np.float32)
    if encoding == "bf16":
        return DeviceBand(K.OBS_BF16, y=bits(y), w=bits(np.where(gone, 0, w).astype(np.float32)))
    half = np.arange(N + PAD) % 2 == 0                                # nodata by the mask, or by w = 0
    return DeviceBand(K.OBS_F32, y=t(y), w=t(np.where(gone & half, 0, w).astype(np.float32)),
                      mask=t((~(gone & ~half)).astype(np.uint8)))


def launch(c, db, N, dev, x=None, **kw):
    """(y_out, w_out, var_out) of one band at the case's states; ld = N + PAD, the padding keeps a sentinel."""
    xd = torch.zeros((c["n"], N + PAD), device=dev)
    xd[:, :N] = torch.from_numpy(c["x"] if x is None else x).to(dev)
    out = torch.full((3, N + PAD), SENTINEL, device=dev)
    K.gp_variance(c["n"], k.gp_spec(c["em"], c["smap"]), xd, out[2], N=N, obs=db, y_out=out[0], w_out=out[1], **kw)
    out = out.cpu().numpy()
    assert (out[:, N:] == SENTINEL).all()
    return out[:, :N]


def check(tag, c, db, out, var_at):
    """``out`` against the float64 reference; ``var_at``: the pixels whose variance was evaluated."""
    s, N = c["em"].signal, out.shape[1]
    yd, wd = (v[:N].cpu().numpy() for v in db.decode())
    seen = wd > 0
    var = c["ref"] * s
    assert seen.any() and (wd[seen] * var[seen] > 0.1).mean() >= 0.25   # else w' = w would pass
    w_ref = 1.0 / (1.0 / wd[seen].astype(np.float64) + var[seen])
    ratio = (np.abs(out[1][seen] - w_ref) / w_ref) / (w_ref * c["allow"] * s + 6 * 2.0 ** -23)
    print(f"MEASURE {tag}: worst error over bound {ratio.max():.3f}, w'/w {np.mean(w_ref / wd[seen]):.3f}")
    assert ratio.max() <= 1.0
    assert np.array_equal(out[0], yd) and not out[1][~seen].any() and not np.signbit(out[1]).any()
    V.check(tag + " var", dict(c, ref=c["ref"][var_at]), out[2][var_at])
    return seen


@pytest.mark.parametrize("encoding", ENCODINGS)
@pytest.mark.parametrize("layout", list(V.LAYOUTS))
def test_host_runner_vs_float64(layout, encoding):
    N = 65
    c, db = V.case(layout, 33, N), band(encoding, N)
    out = launch(c, db, N, "cpu")
    seen = check(f"host {layout} {encoding}", c, db, out, db.decode()[1][:N].numpy() > 0)
    assert not out[2][~seen].any()


def test_config_values():
    assert k.EngineConfig(emulator_uncertainty="inflate").validate().emulator_uncertainty == "inflate"
    with pytest.raises(ValueError, match="emulator_uncertainty"):
        k.EngineConfig(emulator_uncertainty="bogus").validate()
    with pytest.raises(ValueError, match="y_out"):
        K.gp_variance(7, V.emulator("tip", 33), torch.zeros((7, 4)), torch.zeros(4), y_out=torch.zeros(4))
