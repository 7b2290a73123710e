#!/usr/bin/env python
"""Cost of the physical-unit products and the QA layer (``physical=`` / ``qa=``).

Both measurements run in this one process; one JSON line per record, also
appended to ``--record``.

``kernels``: device-event times (median of ``--reps`` calls after warm-up) of
``K.product`` with every parameter selected (``--transform``: all ``neglog``,
the TIP / SAIL kind, by default) and the QA plane with its three inputs, against ``K.marginal`` with the
mean on the same state, precision kind, with the bytes per pixel each moves
and the achieved bandwidth.  n = 7: product reads 35 floats + 3 bytes and
writes 21 floats + 1 byte; marginal reads 35 and writes 14.

    python scripts/bench_product.py kernels --size 10980 --n 7

``e2e``: the tip7 workload of ``bench.py`` (JRC-TIP, 2-band GP operator, LAI
propagator, Gauss-Newton per 256^2 chunk, device-resident rasters) with
``DeviceOutput(uncertainty="marginal")`` -- today's unfused launches -- and
with ``physical=TIP_TRANSFORMS, qa=True`` on top, alternated ``--rounds``
times: ms per step over ``--steps`` timed steps after ``--warmup``.  The
difference is the product pass plus the QA accumulation.

    python scripts/bench_product.py e2e --size 10980 --steps 6 --warmup 2
"""
from __future__ import annotations

import argparse
import datetime as dt
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def emit(rec, record):
    line = json.dumps(rec)
    print(line, flush=True)
    if record:
        with open(record, "a") as f:
            f.write(line + "\n")


def kernels(a):
    import torch

    import kafka_inferenceengine_amd as k
    from kafka_inferenceengine_amd.ops import kernels as K

    if not torch.cuda.is_available():
        raise SystemExit("bench_product kernels needs a GPU")
    dev = torch.device("cuda")
    n, N = a.n, a.size * a.size
    nt = K.ntri(n)
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand((n, N), device=dev, generator=g)
    # SPD by diagonal dominance: |off-diagonal| <= 0.05, diagonal in [1, 2)
    p = torch.empty((nt, N), device=dev)
    diag = {K.ntri(n) - K.ntri(n - j) for j in range(n)}
    for t in range(nt):
        row = torch.rand(N, device=dev, generator=g)
        p[t] = row + 1.0 if t in diag else 0.1 * row - 0.05
    mean = torch.empty((n, N), device=dev)
    unc = torch.empty((n, N), device=dev)
    phys = torch.empty((3 * n, N), device=dev)
    qa = torch.empty(N, dtype=torch.uint8, device=dev)
    status, nobs, nrej = (torch.zeros(N, dtype=torch.uint8, device=dev) for _ in range(3))
    table = [{"neglog": k.ParameterTransform("neglog", scale=2.0, lo=0.0067, hi=1.0),
              "linear": k.ParameterTransform("linear", scale=90.0, lo=0.0, hi=1.0),
              "identity": k.ParameterTransform("identity")}[a.transform]] * n
    z = k.credible_z(0.95)

    def timed(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms), max(ms)

    cases = (("marginal_kernel/precision", 4 * (nt + n), 8 * n,
              lambda: K.marginal(n, x, p, mean, unc, kind="precision")),
             ("product_kernel/precision", 4 * (nt + n) + 3, 12 * n + 1,
              lambda: K.product(n, x, p, table, z, phys=phys, qa=qa, kind="precision", status=status, nobs=nobs,
                                nrej=nrej)),
             ("marginal_kernel/covariance", 8 * n, 8 * n, lambda: K.marginal(n, x, p, mean, unc, kind="covariance")),
             ("product_kernel/covariance", 8 * n + 3, 12 * n + 1,
              lambda: K.product(n, x, p, table, z, phys=phys, qa=qa, kind="covariance", status=status, nobs=nobs,
                                nrej=nrej)))
    for name, rd, wr, fn in cases:
        med, lo, hi = timed(fn)
        assert bool(torch.isfinite(phys[:, ::4097]).all()) and bool(torch.isfinite(unc[:, ::4097]).all())
        emit({"bench": "kernel", "kernel": name, "transform": a.transform if "product" in name else None,
              "size": a.size, "n_params": n, "ms_median": round(med, 4),
              "ms_min": round(lo, 4), "ms_max": round(hi, 4), "reps": a.reps, "read_B_per_px": rd,
              "write_B_per_px": wr, "GB_per_s": round((rd + wr) * N / (med * 1e-3) / 1e9, 1)}, a.record)


def e2e(a):
    import numpy as np
    import torch

    import kafka_inferenceengine_amd as k
    from kafka_inferenceengine_amd.inference import iterate_time_grid

    dev = torch.device(a.device)
    sync = torch.cuda.synchronize if dev.type == "cuda" else (lambda: None)
    mask = np.ones((a.size, a.size), bool)
    n_dates = a.warmup + a.steps + 1
    dates = [dt.datetime(2017, 1, 1) + dt.timedelta(days=16 * i) for i in range(n_dates)]
    grid = [dates[0] - dt.timedelta(days=1)] + [d + dt.timedelta(days=1) for d in dates]
    modes = {"marginal": dict(uncertainty="marginal"),
             "marginal+physical+qa": dict(uncertainty="marginal", physical=k.TIP_TRANSFORMS, qa=True)}
    for rnd in range(a.rounds):
        for mode, kw in modes.items():
            obs = k.SyntheticBHRObservations(mask, dates=dates, n_train=a.n_train, device=dev, n_pool=a.pool,
                                             stream=False, seed=0)
            kf = k.LinearKalman(obs, k.DeviceOutput(k.TIP_PARAMETERS, **kw), mask,
                                k.create_nonlinear_observation_operator, k.TIP_PARAMETERS,
                                state_propagation=k.propagate_information_filter_LAI,
                                device=dev, config=k.EngineConfig(convergence_chunk=[256, 256]))
            kf.set_trajectory_uncertainty(np.array([0, 0, 0, 0, 0, 0, 0.04]))
            state = kf.state_from_prior(k.JRCPrior(k.TIP_PARAMETERS, mask))
            first, ms = True, []
            for i, (t, loc, _) in enumerate(iterate_time_grid(grid, dates)):
                if i >= a.warmup + a.steps:
                    break
                sync()
                t0 = time.perf_counter()
                state = kf.step(t, loc, state, advance=not first, all_dates=dates)
                sync()
                first = False
                if i >= a.warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
            emit({"bench": "e2e", "mode": mode, "round": rnd + 1, "size": a.size, "steps": len(ms),
                  "ms_per_step_median": round(statistics.median(ms), 3), "ms_per_step": [round(v, 3) for v in ms]},
                 a.record)
            del kf, obs, state
            if dev.type == "cuda":
                torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernels", "e2e"])
    ap.add_argument("--size", type=int, default=10980, help="the tile's side")
    ap.add_argument("--n", type=int, default=7, help="kernels: state size")
    ap.add_argument("--transform", default="neglog", choices=["neglog", "linear", "identity"],
                    help="kernels: the kind of every parameter's transform (identity: no logarithm, no clamp -- what "
                         "the pass costs beyond its memory traffic shows against neglog)")
    ap.add_argument("--reps", type=int, default=9, help="kernels: timed calls per kernel (>= 5)")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--n-train", type=int, default=500)
    ap.add_argument("--pool", type=int, default=2, help="e2e: observation dates kept resident")
    ap.add_argument("--device", default="cuda", help="e2e: cuda, or cpu (the host runner: a dry run)")
    ap.add_argument("--record", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least 5")
    kernels(a) if a.what == "kernels" else e2e(a)


if __name__ == "__main__":
    main()
