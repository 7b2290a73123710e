"""Marginal posterior std rasters, sqrt(diag(P)): the per-pixel code on the
host runner against float64, the failure rule, and the engine / outputs / CLI
with ``uncertainty="marginal"``.

Truth is numpy float64 on the float32-rounded input.  The tolerance on the
relative error of a std is ``max(4 n kappa_s, 16) 2^-24`` per pixel, kappa_s
the 2-norm condition number of the pixel's block scaled to unit diagonal
(Cholesky's error does not depend on a diagonal scaling): the (n + 1) u kappa
backward-error bound of the factorisation with a factor for the substitution
and the two roots."""
import datetime as dt
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.engine.state import KFState
from kafka_inferenceengine_amd.input_output.tiff import read_tiff_scaled
from kafka_inferenceengine_amd.ops import kernels as K
from kafka_inferenceengine_amd.utils.blocks import unpack_blocks

from test_engine import _engine, _grid, _setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 3, 4, 7, 10)
U = 2.0 ** -24
SENTINEL = -7.0


def spd_blocks(n, kappa, N, seed):
    """[N, n, n] float64 SPD blocks: random orthogonal Q, a log-uniform spectrum
    pinned at 1 and kappa, rescaled to unit diagonal, then per-parameter units
    exp(U(-3, 3))."""
    rng = np.random.default_rng(seed)
    q, r = np.linalg.qr(rng.standard_normal((N, n, n)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    lam = np.exp(rng.uniform(0.0, np.log(kappa), (N, n)))
    lam[:, 0] = 1.0
    if n > 1:
        lam[:, -1] = kappa
    a = np.einsum("pij,pj,pkj->pik", q, lam, q)
    d = 1.0 / np.sqrt(np.diagonal(a, axis1=1, axis2=2))
    s = d * np.exp(rng.uniform(-3.0, 3.0, (N, n)))
    a = a * s[:, :, None] * s[:, None, :]
    return 0.5 * (a + a.transpose(0, 2, 1))


def pack_rows(blocks, ld):
    """Packed upper-triangle SoA rows [ntri, ld] in float32 (the tail past N is NaN:
    never read)."""
    N, n, _ = blocks.shape
    iu = np.triu_indices(n)
    p = np.full((iu[0].size, ld), np.nan, dtype=np.float32)
    p[:, :N] = blocks[:, iu[0], iu[1]].T
    return p


def blocks_of(packed, n, N):
    """The float64 blocks a kernel sees in packed float32 rows."""
    return unpack_blocks(np.asarray(packed)[:, :N], n).astype(np.float64)


def marginal_truth(blocks):
    """(sqrt(diag(inv A)), bound) per pixel in float64: [N, n], [N]."""
    n = blocks.shape[1]
    sd = np.sqrt(np.diagonal(np.linalg.inv(blocks), axis1=1, axis2=2))
    d = 1.0 / np.sqrt(np.diagonal(blocks, axis1=1, axis2=2))
    kappa_s = np.linalg.cond(blocks * d[:, :, None] * d[:, None, :])
    return sd, np.maximum(4.0 * n * kappa_s, 16.0) * U


def problem(n, kappa, N, seed, device="cpu"):
    """Packed rows with ld = N + 3, a state, and an index map into a plane of N + 5 cells."""
    ld, plane = N + 3, N + 5
    rng = np.random.default_rng(seed + 1)
    p = pack_rows(spd_blocks(n, kappa, N, seed), ld)
    x = rng.standard_normal((n, ld)).astype(np.float32)
    idx = np.sort(rng.permutation(plane)[:N]).astype(np.int64)
    rng.shuffle(idx)
    return (torch.from_numpy(x).to(device), torch.from_numpy(p).to(device), torch.from_numpy(idx).to(device), plane)


def run_marginal(n, x, p, idx, plane, N, kind="precision", mean=True):
    m = torch.full((n, plane), SENTINEL, dtype=torch.float32, device=x.device) if mean else None
    u = torch.full((n, plane), SENTINEL, dtype=torch.float32, device=x.device)
    K.marginal(n, x, p, m, u, idx=idx, N=N, kind=kind)
    return (None if m is None else m.cpu().numpy()), u.cpu().numpy()


def check_kernel(n, kappa, N, seed, device="cpu"):
    """Both kinds against float64 on one problem; sentinel, mean, index map."""
    x, p, idx, plane = problem(n, kappa, N, seed, device)
    A = blocks_of(p.cpu().numpy(), n, N)
    sd, bound = marginal_truth(A)
    ii = idx.cpu().numpy()
    rest = np.setdiff1d(np.arange(plane), ii)
    m, u = run_marginal(n, x, p, idx, plane, N)
    err = np.abs(u[:, ii].T / sd - 1.0)
    print(f"n={n} kappa={kappa:g} N={N}: max err/bound {np.max(err / bound[:, None]):.3f}")
    assert np.all(err <= bound[:, None])
    assert np.array_equal(m[:, ii], x.cpu().numpy()[:, :N])          # the mean: x, bit for bit
    assert np.all(u[:, rest] == SENTINEL) and np.all(m[:, rest] == SENTINEL)
    # marginal >= conditional (1/sqrt(A_jj)), up to the marginal's own error
    cond = 1.0 / np.sqrt(np.diagonal(A, axis1=1, axis2=2))
    assert np.all(u[:, ii].T >= cond * (1.0 - bound[:, None]))
    # covariance kind: the diagonal rows alone; a correctly rounded float32 root of
    # a float32 value is within 2^-24 of the float64 root, 2^-23 leaves one ulp
    mc, uc = run_marginal(n, x, p, idx, plane, N, kind="covariance", mean=False)
    assert mc is None
    assert np.all(np.abs(uc[:, ii].T / np.sqrt(np.diagonal(A, axis1=1, axis2=2)) - 1.0) <= 2 * U)
    assert np.all(uc[:, rest] == SENTINEL)


def check_failure_rule(n, N, seed, device="cpu"):
    """A block that is -I, or holds a NaN, is NaN in all n planes of its pixel and
    nowhere else; a negative covariance diagonal entry is NaN in that entry only."""
    iu = np.triu_indices(n)
    diag_rows = np.nonzero(iu[0] == iu[1])[0]
    for case in ("minus_identity", "nan_entry"):
        x, p, idx, plane = problem(n, 1e3, N, seed, device)
        bad = N // 2
        if case == "minus_identity":
            p[:, bad] = 0.0
            p[diag_rows, bad] = -1.0
        else:
            p[p.shape[0] - 1 if n == 1 else 1, bad] = float("nan")      # (0, 1), the first off-diagonal entry
        _, u = run_marginal(n, x, p, idx, plane, N)
        ii = idx.cpu().numpy()
        nan = np.isnan(u[:, ii])
        assert nan[:, bad].all() and nan.sum() == n, case
        assert np.all(np.isfinite(u[:, np.delete(ii, bad)]) & (u[:, np.delete(ii, bad)] > 0))
    x, p, idx, plane = problem(n, 1e3, N, seed, device)
    bad, j = N // 3, n - 1
    p[diag_rows[j], bad] = -p[diag_rows[j], bad]
    _, u = run_marginal(n, x, p, idx, plane, N, kind="covariance")
    nan = np.isnan(u[:, idx.cpu().numpy()])
    assert nan[j, bad] and nan.sum() == 1


@pytest.mark.parametrize("kappa", [10.0, 1e3, 1e4])
@pytest.mark.parametrize("n", SIZES)
def test_marginal_host_runner_against_float64(n, kappa):
    check_kernel(n, kappa, 257, seed=100 * n + int(np.log10(kappa)))


@pytest.mark.parametrize("n", SIZES)
def test_marginal_failure_rule(n):
    check_failure_rule(n, 257, seed=n)


def test_marginal_argument_checks():
    x, p, idx, plane = problem(3, 10.0, 20, 0)
    u = torch.zeros((3, plane))
    with pytest.raises(ValueError):
        K.marginal(3, x, p, None, u, idx=idx, N=20, kind="variance")
    with pytest.raises(ValueError):
        K.marginal(5, x, p, None, u, idx=idx, N=20)
    with pytest.raises(ValueError):
        K.marginal(3, x, p[:5], None, u, idx=idx, N=20)
    with pytest.raises(ValueError):
        K.marginal(3, x, p, None, torch.zeros((3, 10)), N=20)            # plane < N without an index map
    with pytest.raises(TypeError):
        K.marginal(3, x, p.double(), None, u, idx=idx, N=20)


# ---------------------------------------------------------------- engine
def engine_pair(form, make_engine, device="cpu"):
    """One run with marginal rasters and one with today's non-fused conditional
    output: the analyses are the same launches, so the states are equal bit for
    bit and only the uncertainty planes differ."""
    res = []
    for kw, cfg in ((dict(uncertainty="marginal"), {}), ({}, dict(fuse_output=False))):
        out = k.DeviceOutput(k.TIP_PARAMETERS, keep_history=True, **kw)
        kf, run = make_engine(out, analysis_form=form, **cfg)
        st = run(kf)
        res.append((st, out, [h.get("gn_iterations") for h in kf.history], kf))
    (sm, om, gm, kfm), (sc, oc, gc, _) = res
    assert sm.kind == sc.kind == ("covariance" if form == "gain" else "precision")
    assert torch.equal(sm.x, sc.x) and torch.equal(sm.P, sc.P) and gm == gc
    assert sorted(om.history) == sorted(oc.history) and len(om.history) >= 2
    mask = kfm.partition.local_mask.reshape(-1)
    for t in om.history:
        assert torch.equal(om.history[t][0], oc.history[t][0])           # the mean raster
        u, uc = om.history[t][1].cpu().numpy(), oc.history[t][1].cpu().numpy()
        assert np.all(np.isfinite(u[:, mask]) & (u[:, mask] > 0)) and np.all(u[:, ~mask] == 0)
        assert not np.array_equal(u, uc)
    # the last date's raster against the float64 marginal of the final state
    n, N = 7, sm.N
    u = om.history[max(om.history)][1].cpu().numpy()[:, mask]
    A = blocks_of(sm.P.cpu().numpy(), n, N)
    if form == "gain":
        sd, bound = np.sqrt(np.diagonal(A, axis1=1, axis2=2)), np.full(N, 2 * U)
    else:
        sd, bound = marginal_truth(A)
    err = np.abs(u.T / sd - 1.0)
    print(f"{form}: last date max err/bound {np.max(err / bound[:, None]):.3f}")
    assert np.all(err <= bound[:, None])
    # LinearKalman.unc(kind="marginal") is the same pass without the scatter
    assert np.array_equal(kfm.unc(sm, kind="marginal").cpu().numpy(), u)
    return om, kfm, sm


def _cpu_engine(seed):
    mask, obs, prior, x0, Pinv, Q = _setup(seed=seed)
    grid = _grid(4)

    def make(out, **cfg):
        return _engine(mask, obs, Q, out=out, **cfg), lambda kf: kf.run(grid, x0, None, Pinv)
    return make, mask, grid


@pytest.mark.parametrize("form", ["information", "gain"])
def test_engine_marginal_output_equals_non_fused_run(form):
    make, _, _ = _cpu_engine(seed=6)
    engine_pair(form, make)


def test_marginal_with_spatial_prior_and_bad_values_raise():
    mask, obs, prior, x0, Pinv, Q = _setup(seed=9)
    out = k.DeviceOutput(k.TIP_PARAMETERS, uncertainty="marginal")
    kf = _engine(mask, obs, Q, out=out, spatial_gamma=50.0, spatial_params=[6], jacobi_sweeps=4)
    with pytest.raises(ValueError, match="spatial"):
        kf.run(_grid(3), x0, None, Pinv)
    for cls, args in ((k.DeviceOutput, (k.TIP_PARAMETERS,)), (k.KafkaOutputMemory, (k.TIP_PARAMETERS,))):
        with pytest.raises(ValueError, match="uncertainty"):
            cls(*args, uncertainty="joint")
    with pytest.raises(ValueError, match="uncertainty"):
        k.KafkaOutput(k.TIP_PARAMETERS, None, "", "unused", uncertainty="joint")
    with pytest.raises(ValueError):
        _engine(mask, obs, Q).unc(KFState.empty(7, int(mask.sum()), torch.device("cpu")), kind="joint")


def test_kafka_output_marginal_files_equal_device_rasters(tmp_path):
    make, mask, grid = _cpu_engine(seed=5)
    ref = k.DeviceOutput(k.TIP_PARAMETERS, keep_history=True, uncertainty="marginal")
    kf, run = make(ref)
    run(kf)
    out = k.KafkaOutput(k.TIP_PARAMETERS, [500000., 10., 0., 4000000., 0., -10.], "EPSG:32630", str(tmp_path / "f32"),
                        uncertainty="marginal", encoder="host")
    kf, run = make(out)
    st = run(kf)
    out.flush()
    assert out.writer_stats()["uncertainty"] == "marginal"
    assert k.KafkaOutput(k.TIP_PARAMETERS, None, "", str(tmp_path / "c")).writer_stats()["uncertainty"] == "conditional"
    assert len(out.written) == 14 * len(ref.history)
    for ts, (m, u) in ref.history.items():
        for p, name in enumerate(k.TIP_PARAMETERS):
            core = f"{name}_{ts.strftime('A%Y%j')}"
            arr, info = k.read_tiff(tmp_path / "f32" / f"{core}.tif")
            assert np.array_equal(arr.reshape(-1), m[p].numpy()) and "uncertainty" not in info
            arr, info = k.read_tiff(tmp_path / "f32" / f"{core}_unc.tif")
            assert np.array_equal(arr.reshape(-1), u[p].numpy()) and info["uncertainty"] == "marginal"
    # uint16 samples: a pixel whose precision is not SPD is NaN, written as nodata 65535
    rg = {p: (-2.0, 8.0) for p in k.TIP_PARAMETERS}
    urg = {p: (0.0, 20.0) for p in k.TIP_PARAMETERS}
    o16 = k.KafkaOutput(k.TIP_PARAMETERS, [500000., 10., 0., 4000000., 0., -10.], "EPSG:32630", str(tmp_path / "u16"),
                        uncertainty="marginal", encoder="host", sample_type="uint16", ranges=rg, unc_ranges=urg)
    P = st.P.clone()
    bad = 17
    P[:, bad] = 0.0
    P[[K.ntri(7) - K.ntri(7 - j) for j in range(7)], bad] = -1.0
    ts = grid[-1]
    o16.dump_state(ts, KFState(st.x, P, st.kind, st.N), kf)
    o16.flush()
    cell = np.flatnonzero(mask.reshape(-1))[bad]
    last = ref.history[max(ref.history)][1].numpy()
    for p, name in enumerate(k.TIP_PARAMETERS):
        raw, info = k.read_tiff(tmp_path / "u16" / f"{name}_{ts.strftime('A%Y%j')}_unc.tif")
        assert raw.dtype == np.uint16 and info["uncertainty"] == "marginal" and info["scale"] is not None
        raw = raw.reshape(-1)
        assert raw[cell] == 65535 and np.count_nonzero(raw == 65535) == 1
        val, _ = read_tiff_scaled(tmp_path / "u16" / f"{name}_{ts.strftime('A%Y%j')}_unc.tif")
        keep = np.arange(raw.size) != cell
        assert np.all(np.abs(val.reshape(-1)[keep] - np.clip(last[p][keep], 0.0, 20.0)) <= 0.5 * info["scale"] * 1.001)


def test_reference_signature_outputs_marginal(tmp_path):
    """dump_data (the reference API: scipy blocks): float64 diag(inv(P^-1)), or
    diag(P) where the covariance is handed in."""
    from kafka_inferenceengine_amd.utils.blocks import blocks_to_sparse
    n, N = 3, 12
    A = blocks_of(pack_rows(spd_blocks(n, 1e3, N, 4), N), n, N)
    sd, _ = marginal_truth(A)
    x = np.arange(n * N, dtype=np.float64)
    mem = k.KafkaOutputMemory(["a", "b", "c"], uncertainty="marginal")
    t = dt.datetime(2017, 1, 1)
    mem.dump_data(t, x, None, blocks_to_sparse(A), None, n)
    assert np.allclose(np.stack([mem.output[t][p + "_unc"] for p in "abc"], 1), sd, rtol=1e-9)
    mem.dump_data(t, x, blocks_to_sparse(np.linalg.inv(A)), None, None, n)
    assert np.allclose(np.stack([mem.output[t][p + "_unc"] for p in "abc"], 1), sd, rtol=1e-9)
    B = A.copy()
    B[5] = -np.eye(n)
    mem.dump_data(t, x, None, blocks_to_sparse(B), None, n)
    got = np.stack([mem.output[t][p + "_unc"] for p in "abc"], 1)
    assert np.isnan(got[5]).all() and np.allclose(np.delete(got, 5, 0), np.delete(sd, 5, 0), rtol=1e-9)
    mask = np.ones((3, 4), bool)
    out = k.KafkaOutput(["a", "b", "c"], None, "", str(tmp_path), uncertainty="marginal", asynchronous=False)
    out.dump_data(t, x, None, blocks_to_sparse(A), mask, n)
    arr, info = k.read_tiff(tmp_path / f"b_{t.strftime('A%Y%j')}_unc.tif")
    assert np.array_equal(arr.reshape(-1), sd[:, 1].astype(np.float32)) and info["uncertainty"] == "marginal"


def test_cli_run_out_unc_marginal(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="4")
    r = subprocess.run([sys.executable, "-m", "kafka_inferenceengine_amd", "run", "--sensor", "bhr", "--size", "24",
                        "20", "--steps", "2", "--n-train", "40", "--device", "cpu", "--out", str(tmp_path / "tif"),
                        "--out-unc", "marginal"], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["timesteps"] == 2 and rec["finite"] and rec["output"]["uncertainty"] == "marginal"
    files = sorted(os.listdir(tmp_path / "tif"))
    assert len(files) == 2 * 2 * 7
    unc = [f for f in files if f.endswith("_unc.tif")]
    assert len(unc) == 14
    for f in unc:
        arr, info = k.read_tiff(tmp_path / "tif" / f)
        assert info["uncertainty"] == "marginal" and np.isfinite(arr).all() and (arr > 0).all()
