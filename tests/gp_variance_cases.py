"""Shared cases of the GP predictive-variance tests (test_gp_variance.py on the CPU,
test_gpu_gp_variance.py on the device): emulators, states drawn in the design box
stretched by 20 % per side, the float64 reference and the allowance.

Allowance, in units of the signal variance s: 4 x the error of a plain NumPy float32
evaluation of the whitened form on the same inputs (k^ and W^ rounded to float32, one
matmul, square and sum in float64), floor 2^-20.  4 x is the margin a matrix-core kernel
gets over its float32 counterpart (test_gpu_hessian_mfma.py)."""
import datetime as dt
import functools

import numpy as np
from scipy.linalg import solve_triangular

import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.models import gp as G

LAYOUTS = {"tip": (4, 7, [0, 1, 6, 2]), "prosail": (10, 10, list(range(10)))}   # D, n_params, state map
TS = (31, 33, 500)      # below and just past one 32-point chunk, the shipped size


@functools.lru_cache(maxsize=None)
def emulator(layout, T):
    return G.make_tip_emulators(n_train=T)[0] if layout == "tip" else \
        G.make_prosail_emulators(n_bands=1, n_train=T)[0]


def whitened(em):
    return np.sqrt(em.signal) * solve_triangular(em.cholesky(), np.eye(em.n_train), lower=True)


@functools.lru_cache(maxsize=None)
def case(layout, T, N):
    D, n, smap = LAYOUTS[layout]
    em = emulator(layout, T)
    rng = np.random.default_rng([T, N, D])
    lo, hi = em.inputs.min(0), em.inputs.max(0)
    X = (lo - 0.2 * (hi - lo) + 1.4 * (hi - lo) * rng.random((N, D))).astype(np.float32)
    x = rng.normal(size=(n, N)).astype(np.float32)
    x[smap] = X.T
    X = X.astype(np.float64)
    ref = em.variance(X) / em.signal
    u = (em._kernel(X)[2] / em.signal).astype(np.float32) @ whitened(em).T.astype(np.float32)
    e32 = np.abs(np.maximum(1.0 - (u.astype(np.float64) ** 2).sum(1), 0.0) - ref).max()
    return dict(em=em, n=n, smap=smap, x=x, X=X, ref=ref, e32=e32, allow=max(4.0 * e32, 2.0 ** -20))


def check(tag, c, var):
    """``var`` (float32, in s units times s) against the float64 reference, within the allowance."""
    err = np.abs(np.asarray(var, dtype=np.float64) / c["em"].signal - c["ref"]).max()
    print(f"MEASURE {tag}: err {err:.3e} s, float32 {c['e32']:.3e} s, allowance {c['allow']:.3e} s, "
          f"ratio {err / c['allow']:.3f}")
    assert err <= c["allow"]


def engine_run(dev, **cfg):
    """A 2-date JRC-TIP run on a 16 x 16 tile; returns the engine and the final state."""
    mask = np.ones((16, 16), bool)
    obs = k.SyntheticBHRObservations(mask, n_train=80, stream=False, n_pool=5, device=dev, seed=0, field_cell=8)
    x0, Pinv = k.JRCPrior(k.TIP_PARAMETERS, mask).process_prior(None)
    kf = k.LinearKalman(obs, None, mask, k.create_nonlinear_observation_operator, k.TIP_PARAMETERS,
                        state_propagation=k.propagate_information_filter_LAI, device=dev, config=k.EngineConfig(**cfg))
    kf.set_trajectory_model()
    kf.set_trajectory_uncertainty(np.zeros_like(x0))
    return kf, kf.run([dt.datetime(2017, 1, 1), dt.datetime(2017, 1, 17)], x0, None, Pinv)
