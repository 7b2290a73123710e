"""Structure-aware solve of the JRC-TIP state (kf_core.h StructTip, ops/kernels.py
tip_structure) on the host runner: with the JRC prior the forecast precision and
every analysis precision are exactly zero in 8 of the 21 off-diagonal entries,
the masked Cholesky / solve / symv skip those operations, and the results are
the dense solve's bit for bit.  A prior with a non-zero outside the pattern
takes the dense path."""
from __future__ import annotations

import datetime as dt

import numpy as np
import torch

import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.inference.kf_tools import make_partial_prior_propagator
from kafka_inferenceengine_amd.ops import kernels as K


def _mask():
    mask = np.ones((24, 20), bool)
    mask[5:9, 6:13] = False
    return mask


def _run(variant, prior_cinv=None):
    mask = _mask()
    grid = [dt.datetime(2017, 1, 1) + dt.timedelta(days=16 * i) for i in range(4)]
    old = K.DEFAULT_VARIANT
    K.DEFAULT_VARIANT = variant
    K.STRUCT_LAUNCHES.update(tip=0, dense=0)
    try:
        obs = k.SyntheticBHRObservations(mask, n_train=40, device="cpu", stream=False, n_pool=3, field_cell=8,
                                         cloud_fraction=0.3)
        prop = k.propagate_information_filter_LAI
        if prior_cinv is not None:   # the LAI propagator resetting to another prior precision
            prop = make_partial_prior_propagator(k.tip_prior()[0], prior_cinv, (6,))
        kf = k.LinearKalman(obs, None, mask, k.create_nonlinear_observation_operator, k.TIP_PARAMETERS,
                            device="cpu", state_propagation=prop)
        kf.set_trajectory_uncertainty(np.array([0, 0, 0, 0, 0, 0, 0.04]))
        st = kf.run(grid, kf.state_from_prior(k.JRCPrior(k.TIP_PARAMETERS, mask)), None, None)
        return dict(x=st.x.clone(), P=st.P.clone(), status=kf.last_status.clone(),
                    norms=[h.get("norms") for h in kf.history], iters=[h.get("gn_iterations") for h in kf.history],
                    launches=dict(K.STRUCT_LAUNCHES))
    finally:
        K.DEFAULT_VARIANT = old


def _same(a, b):
    assert a["iters"] == b["iters"] and a["norms"] == b["norms"]
    assert torch.equal(a["x"], b["x"]) and torch.equal(a["P"], b["P"]) and torch.equal(a["status"], b["status"])


def test_structure_mask_is_the_tip_pattern():
    """The mask of ops/kernels.py is the complement of the entries the two band
    maps {0, 1, 6, 2}, {3, 4, 6, 5} and the prior's (2, 5) pair touch, and the
    JRC prior passes the host check with both flags."""
    on = {(min(i, j), max(i, j)) for m in k.TIP_BAND_MAPPER for i in m for j in m if i != j} | {(2, 5)}
    off = {(i, j) for i in range(7) for j in range(i + 1, 7)} - on
    assert off == set(K.TIP_ZERO_ENTRIES)
    Pi = k.tip_prior()[2]
    assert all(Pi[i, j] == 0.0 and Pi[j, i] == 0.0 for i, j in K.TIP_ZERO_ENTRIES)


def test_host_runner_sparse_equals_dense():
    sparse = _run(K.Variant.DEFAULT)
    dense = _run(K.Variant.DENSE_SOLVE)
    assert sparse["launches"]["tip"] > 0 and sparse["launches"]["dense"] == 0, sparse["launches"]
    assert dense["launches"]["tip"] == 0 and dense["launches"]["dense"] > 0, dense["launches"]
    assert np.isfinite(sparse["x"].numpy()).all()
    _same(sparse, dense)


def test_prior_outside_the_pattern_takes_the_dense_path():
    cov = np.array(k.tip_prior()[1], dtype=np.float64)
    cov[0, 4] = cov[4, 0] = 0.3 * np.sqrt(cov[0, 0] * cov[4, 4])   # couples w_vis and x_nir: outside the mask
    cinv = np.linalg.inv(cov)
    assert cinv[0, 4] != 0.0
    default = _run(K.Variant.DEFAULT, cinv)
    oracle = _run(K.Variant.DENSE_SOLVE, cinv)
    assert default["launches"]["tip"] == 0 and default["launches"]["dense"] > 0, default["launches"]
    _same(default, oracle)
