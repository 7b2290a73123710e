"""The kernels the launch plan (csrc/kf_plan.h) selects, launched: every GP plan the CPU enumeration
(test_launch_plan.py) reaches through ops/kernels.py with real operands is launched once on 130 pixels
(two full waves and a two-lane tail, one workgroup), with emulators of 32 and 160 training points (1 and
5 chunks of 32: either side of the launchers' `small` threshold).  Each launch must take the expected
kernel (the plan kernels.py recorded) and agree with the host runner of the same per-pixel code under the
comparison of test_gpu_mfma.py::test_gp_mfma_analysis_vs_oracle_and_valu: 1e-4 relative on x (scale
|x| + 0.05), equal status bytes.

Measured on an MI355X: the largest error is 7.4e-5 (JRC-TIP, SPEC_PROP_REG*), the generic VALU kernel
`analysis_kernel<7, 0, 0>` is at 6.1e-5 from the host runner of the same code; the 10-parameter launches
are within 3.3e-5 and the 3-parameter ones within 1.3e-5."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import pytest
import torch

import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.models.gp import GaussianProcessEmulator
from kafka_inferenceengine_amd.models.priors import sail_prior
from kafka_inferenceengine_amd.ops import kernels as K
from kafka_inferenceengine_amd.utils.blocks import pack_matrix

import kernel_cases as C

pytestmark = pytest.mark.gpu

N = 130
TOL = 1e-4
V = K.Variant
DIAG_ROW = 27   # tri(7, 6, 6): the propagated parameter's diagonal entry


@functools.lru_cache(maxsize=None)
def case(kind, n_train, dn16):
    """Inputs of one state size: "tip" (7 parameters, the two JRC-TIP bands), "prosail" (10, two
    full-state bands) or "small" (3, one full-state band)."""
    if kind == "tip":
        return C.tip_problem(N=N, seed=3, n_train=n_train, dn16=dn16)
    rng = np.random.default_rng(11)
    if kind == "prosail":
        n, ems = 10, k.make_prosail_emulators(n_bands=2, n_train=n_train, seed=6)
        mu, cov, _ = sail_prior()
        sig = np.maximum(np.sqrt(np.diag(cov)), 0.05)
    else:
        n, mu, sig = 3, np.full(3, 0.5), np.full(3, 0.15)
        ems = [GaussianProcessEmulator.synthetic(lambda X: 0.3 + 0.2 * np.sin(2 * X[:, 0]) + 0.15 * X[:, 1] * X[:, 2],
                                                 np.zeros(3), np.ones(3), n_train, 5, name="small")]
    # a forecast near the prior mean and a linearisation point near the forecast, as a Gauss-Newton iterate
    # is and as test_gpu_mfma.py's gp_problem has it (2 % of the box there).  The host runner is the
    # reference, so the inputs must leave it well inside the 1e-4 it is compared under: against float64
    # (inference.analysis_blocks over predict) it is within 1.9e-5 in every 10- and 3-parameter case.
    # Linearised 0.5 sig from the forecast, exp(-LAI/2) (mean 0.135, sig 0.5) starts below 0 in a third of
    # the pixels and the step brings it back through 0, where the host runner alone was 1.14e-4 off.
    xf = mu + rng.normal(size=(N, n)) * sig * 0.05
    x = xf + rng.normal(size=(N, n)) * sig * 0.05
    Pf = np.broadcast_to(np.diag(1.0 / sig ** 2), (N, n, n)) + 0.0
    raw = []
    for em in ems:
        y = em.predict(x)[0]
        # noise at the uncertainty the band declares: kernel_cases.device_bands' DN16 model, or w = 1e4
        y = np.clip(y + rng.normal(size=N) * (np.maximum(0.05 * y, 2.5e-3) if dn16 else 0.01), 0.01, 1.0)
        valid = rng.random(N) > 0.2
        if dn16:
            raw.append(dict(dn=np.where(valid, np.clip(np.round(y / 1e-4), 1, 32767), 0).astype(np.int16)))
        else:
            raw.append(dict(y=y.astype(np.float32), w=np.where(valid, 1e4, 0.0).astype(np.float32)))
    specs = [k.gp_spec(em, np.arange(n)) for em in ems]
    return dict(x=x, xf=xf, Pf=Pf, specs=specs, raw=raw, dn16=dn16, N=N, n=n, mu=mu, sig=sig)


def band_table(prob, device, tables):
    """tables "global": the bands' tables read from global memory, as for tables too large for the LDS."""
    tab = C.table(prob, device)
    assert tab.gpm_frags > 0, "matrix-core tables not attached"
    if tables == "global":
        tab = dataclasses.replace(tab, gpm_frags=0, gpm_global=True)
    return tab


def forecast(prob, device, cov=False):
    """Fused-forecast arguments: one propagated parameter, the others reset to the prior."""
    n = prob["n"]
    if n == 7:
        spec = C.containment_spec(n)
    else:
        spec = {"mode": 1, "m": np.ones(n), "q": np.full(n, 0.04), "prop_mask": 1, "reset_mean": prob["mu"],
                "reset_cinv": pack_matrix(np.diag(1.0 / prob["sig"] ** 2))}
    pa = np.linalg.inv(prob["Pf"]) if cov else prob["Pf"]
    return K.prop_args(n, spec, C.soa(prob["xf"], device), C.packed(pa, device), fused=True)


def analysis(prob, device, variant=None, prop=False, tables="lds", rows="all", out="none", reg=False, fast=True):
    n = prob["n"]
    tab = band_table(prob, device, tables)
    xo = torch.zeros((n, N), device=device)
    ao = None if rows == "none" else torch.zeros((n * (n + 1) // 2, N), device=device)
    st = torch.zeros(N, dtype=torch.uint8, device=device)
    unc = torch.zeros((n, N), device=device)
    o = None if out == "none" else (torch.zeros((n, N), device=device) if out == "mean" else None, unc, None)
    kw = dict(out=o, variant=variant, fast=fast, a_rows=(1 << DIAG_ROW) if rows == "diag" else None)
    if reg:
        kw.update(out=(None, unc, None),
                  reg=dict(gamma=2.0, mask=1 << 6, geo={"w": 13, "h": 10, "halo": 0, "n_up": 0}, nbr=None,
                           v_out=torch.zeros((n, N), device=device)))
    K.LAST_PLAN = None
    if prop:
        K.analysis(n, tab, None, None, None, xo, ao, None, st, None, prop=forecast(prob, device), **kw)
    else:
        K.analysis(n, tab, C.soa(prob["x"], device), C.soa(prob["xf"], device), C.packed(prob["Pf"], device), xo, ao,
                   None, st, None, **kw)
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()
    return K.LAST_PLAN, xo.cpu().numpy(), st.cpu().numpy()


def gain(prob, device, variant=None, prop=False, tables="lds"):
    """-> (the plan of the argument block kernels.py launched, x, status)."""
    n = prob["n"]
    tab = band_table(prob, device, tables)
    xo = torch.zeros((n, N), device=device)
    po = torch.zeros((n * (n + 1) // 2, N), device=device)
    st = torch.zeros(N, dtype=torch.uint8, device=device)
    ext, plans = K.ext(), []
    real, old = ext.gain, K.DEFAULT_VARIANT

    def recording(np_, a, *rest):
        plans.append(ext.gain_plan(np_, a))
        return real(np_, a, *rest)

    ext.gain, K.DEFAULT_VARIANT = recording, (old if variant is None else variant)
    try:
        if prop:
            K.gain(n, tab, None, None, None, xo, po, st, prop=forecast(prob, device, cov=True))
        else:
            K.gain(n, tab, C.soa(prob["x"], device), C.soa(prob["xf"], device),
                   C.packed(np.linalg.inv(prob["Pf"]), device), xo, po, st)
    finally:
        ext.gain, K.DEFAULT_VARIANT = real, old
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()
    return plans[-1], xo.cpu().numpy(), st.cpu().numpy()


def mfma(n, d, obs, layout, il, spec, minw=3, mixlo=False):
    return f"analysis_mfma_{'mixlo_' if mixlo else ''}kernel<{n}, {d}, {obs}, 256, {minw}, {layout}, {il}, {spec}>"


def launches():
    """(id, launch function, keyword arguments, expected kernel)."""
    out = []

    def add(fn, kind, n_train, dn16, name, **kw):
        what = "-".join([fn.__name__, kind, str(n_train), "dn16" if dn16 else "f32"] +
                        [f"{a}={getattr(b, 'name', b)}" for a, b in kw.items()])
        out.append(pytest.param(fn, (kind, n_train, dn16), kw, name, id=what))

    for dn16 in (True, False):
        obs = K.OBS_DN16 if dn16 else K.OBS_F32
        # JRC-TIP, no forecast fused (the first date)
        add(analysis, "tip", 160, dn16, mfma(7, 4, obs, 1, "true", 0))
        add(analysis, "tip", 160, dn16, mfma(7, 4, obs, 1, "false", 0), variant=V.BLOCK_ORDER)
        add(analysis, "tip", 160, dn16, mfma(7, 4, obs, 0, "false", 0), variant=V.RUNTIME_LAYOUT)
        add(analysis, "tip", 160, dn16, f"analysis_kernel<7, 4, {obs}, 4, false>", variant=V.VALU_ORACLE)
        add(analysis, "tip", 160, dn16, "analysis_kernel<7, 0, 0, 4, false>", fast=False)
        add(gain, "tip", 160, dn16, f"gain_mfma_kernel<7, 4, {obs}>")
        add(gain, "tip", 160, dn16, f"gain_kernel<7, 4, {obs}>", variant=V.VALU_ORACLE)
        # 10 parameters, LDS and global tables
        add(analysis, "prosail", 32, dn16, mfma(10, 10, obs, 0, "true", 0, minw=1))
        add(analysis, "prosail", 32, dn16, mfma(10, 10, obs, 0, "false", 0, minw=1), variant=V.BLOCK_ORDER)
        add(analysis, "prosail", 32, dn16, f"analysis_kernel<10, 10, {obs}, 4, false>", variant=V.VALU_ORACLE)
        add(analysis, "prosail", 160, dn16, f"analysis_mfma_g_kernel<10, 10, {obs}, false, true, 0>", tables="global")
        add(gain, "prosail", 160, dn16, f"gain_mfma_g_kernel<10, 10, {obs}>", tables="global")
        add(gain, "prosail", 32, dn16, f"gain_kernel<10, 10, {obs}>")
        # 3 parameters, one band
        add(analysis, "small", 32, dn16, mfma(3, 3, obs, 0, "false", 0))
        add(analysis, "small", 160, dn16, mfma(3, 3, obs, 0, "true", 0), variant=V.BLOCK_ORDER)
        add(analysis, "small", 32, dn16, f"analysis_kernel<3, 3, {obs}, 4, false>", variant=V.VALU_ORACLE)
    add(gain, "small", 32, True, "gain_kernel<3, 0, 0>")
    add(analysis, "tip", 160, True, mfma(7, 4, 2, 1, "true", 0, mixlo=True), variant=V.MIXLO_SPLIT)
    add(gain, "tip", 160, True, "gain_mfma_mixlo_kernel<7, 4, 2>", variant=V.MIXLO_SPLIT)
    # JRC-TIP with the forecast fused: 32 training points are a small emulator (SPEC_PROP_PF*), 160 not
    for n_train, small in ((32, True), (160, False)):
        add(analysis, "tip", n_train, True, "analysis_tip_sl_kernel<true, 2, 0>", prop=True)
        add(analysis, "tip", n_train, True, mfma(7, 4, 2, 1, "true", 6 if small else 4), prop=True, variant=V.LOOPED_TIP)
        add(analysis, "tip", n_train, True, mfma(7, 4, 2, 1, "true", 3 if small else 1), prop=True, variant=V.DENSE_SOLVE)
        add(analysis, "tip", n_train, True, mfma(7, 4, 2, 1, "true", 6 if small else 4, mixlo=True), prop=True,
            variant=V.MIXLO_SPLIT)
    add(analysis, "tip", 160, True, mfma(7, 4, 2, 1, "true", 0), prop=True, variant=V.GENERIC_SPEC)
    add(analysis, "tip", 160, True, mfma(7, 4, 2, 1, "false", 0), prop=True, variant=V.BLOCK_ORDER)
    add(analysis, "tip", 160, True, mfma(7, 4, 2, 0, "false", 0), prop=True, variant=V.RUNTIME_LAYOUT)
    add(analysis, "tip", 160, True, "analysis_kernel<7, 4, 2, 4, false>", prop=True, variant=V.VALU_ORACLE)
    add(analysis, "tip", 160, True, mfma(7, 4, 2, 1, "true", 5), prop=True, reg=True)
    add(analysis, "tip", 160, True, mfma(7, 4, 2, 1, "true", 2), prop=True, reg=True, variant=V.DENSE_SOLVE)
    add(gain, "tip", 160, True, "gain_mfma_kernel<7, 4, 2>", prop=True)
    # the other eight shapes of the straight-line kernel (stored rows x fused output rasters)
    for r, rows in enumerate(("none", "diag", "all")):
        for o, outs in enumerate(("none", "unc", "mean")):
            if (rows, outs) != ("all", "none"):
                add(analysis, "tip", 32, True, f"analysis_tip_sl_kernel<true, {r}, {o}>", prop=True, rows=rows, out=outs)
    # 10 parameters with global tables: the forecast fused, the prefetch and block-order variants, the other split
    g = "analysis_mfma_g_kernel<10, 10, 2, "
    add(analysis, "prosail", 160, True, g + "false, true, 1>", tables="global", prop=True)
    add(analysis, "prosail", 160, True, g + "false, false, 0>", tables="global", variant=V.BLOCK_ORDER)
    add(analysis, "prosail", 160, True, g + "true, false, 0>", tables="global", variant=V.GT_PREFETCH)
    add(analysis, "prosail", 160, True, "analysis_mfma_g_mixlo_kernel<10, 10, 2, false, true, 0>", tables="global",
        variant=V.MIXLO_SPLIT)
    add(analysis, "prosail", 160, True, "analysis_mfma_g_mixlo_kernel<10, 10, 2, false, true, 1>", tables="global",
        prop=True, variant=V.MIXLO_SPLIT)
    add(gain, "prosail", 160, True, "gain_mfma_g_mixlo_kernel<10, 10, 2>", tables="global", variant=V.MIXLO_SPLIT)
    add(gain, "prosail", 160, True, "gain_kernel<10, 10, 2>", tables="global", variant=V.VALU_ORACLE)
    return out


LAUNCHES = launches()


def test_the_launches_are_distinct_table_lines():
    names = [p.values[3] for p in LAUNCHES]
    assert len(set(names)) >= 50 and set(names) <= set(K.ext().launch_table())


@pytest.mark.parametrize("fn,problem,kw,kernel", LAUNCHES)
def test_planned_kernel_runs_and_agrees_with_the_host_runner(cuda, fn, problem, kw, kernel):
    prob = case(*problem)
    plan, x, st = fn(prob, cuda, **kw)
    assert plan is not None and plan["name"] == kernel, plan
    _, xr, sr = fn(prob, "cpu", **kw)
    err = np.max(np.abs(x - xr) / (np.abs(xr) + 0.05))
    print(f"{kernel}: x err against the host runner {err:.2e}")
    assert np.isfinite(xr).all() and err < TOL, err
    assert np.array_equal(st, sr)
