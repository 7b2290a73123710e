"""Cases of tests/test_gpu_gp_operator_mfma.py: two GP bands on an n-parameter state, each with its own state
map and emulator size, observed through C.nongp_case's F32 and DN16 planes (both mask some pixels), against the
float64 emulator within the project's gp_operator bound (tests/test_gpu_aux.py: value 5e-6, gradient 5e-5)."""
import functools

import numpy as np

import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.engine.bands import RecordCache, build_table
from kafka_inferenceengine_amd.models.gp import GaussianProcessEmulator
from kafka_inferenceengine_amd.ops import kernels as K

import kernel_cases as C

ATOL_VALUE, ATOL_GRAD = 5e-6, 5e-5
MAPS_10_4 = ((0, 3, 9, 5), (2, 4, 6, 8))
MAPS_7_MIXED = (tuple(range(7)), tuple(k.TIP_BAND_MAPPER[0]))   # a d = 7 and a d = 4 band in one call


@functools.lru_cache(maxsize=None)
def emulator(d, T=64):
    return GaussianProcessEmulator.synthetic(
        lambda X: 0.3 + 0.2 * np.sin(2 * X[:, 0]) + 0.15 * X[:, 1 % d] * X[:, d - 1], np.zeros(d), np.ones(d), T, 5)


def case(n, maps, N, T=(64, 64), dark=None):
    """-> (x0 [N, n], evals [(H0, h, y, w)] float64, table(dev, pad, cache)); C.small_gp's target with T[b]
    training points per band; ``dark``: a pixel slice in which both bands are masked."""
    c = C.nongp_case(n, N, (("gp", K.OBS_F32), ("gp", K.OBS_DN16)))
    x0 = c["x0"].copy()
    raws = [{key: None if v is None else v.copy() for key, v in r.items()} for r in c["raws"]]
    ws = [c["evals"][b][3].copy() for b in range(2)]
    if dark is not None:
        raws[0]["w"][dark], raws[1]["dn"][dark] = 0.0, 0
        ws[0][dark] = ws[1][dark] = 0.0
    specs, evals = [], []
    for b, mp in enumerate(map(list, maps)):
        em = emulator(len(mp), T[b])
        specs.append(k.gp_spec(em, mp))
        H, dH = em.predict(x0[:, mp])
        h = np.zeros((N, n))
        h[:, mp] = dH
        evals.append((H, h, c["evals"][b][2], ws[b]))
    return x0, evals, lambda dev, pad, cache=None: build_table(
        specs, [C.device_band(c["bands"][b][1], raws[b], N + pad, dev) for b in range(2)], n, cache or RecordCache(),
        dev)


def errors(tag, evals, n, h0, h):
    """Worst error / bound (value, gradient) over the observed pixels; masked ones hold +0.0 in h0 and all n rows."""
    worst = [0.0, 0.0]
    for b, (H, hr, _, w) in enumerate(evals):
        on = w > 0
        g = np.column_stack([h0[b], h[b * n:(b + 1) * n].T]).astype(np.float64)
        assert len(w) < 63 or (~on).any(), "the case must mask some pixels"
        assert not g[~on].any() and not np.signbit(g[~on]).any(), (tag, b)
        worst = [max(worst[0], np.abs(g[on, 0] - H[on]).max(initial=0.0) / ATOL_VALUE),
                 max(worst[1], np.abs(g[on, 1:] - hr[on]).max(initial=0.0) / ATOL_GRAD)]
    print(f"MEASURE gp_operator mfma {tag}: worst error / bound value {worst[0]:.3f} gradient {worst[1]:.3f}")
    return worst
