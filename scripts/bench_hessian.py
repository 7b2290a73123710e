#!/usr/bin/env python
"""Cost of K6, the Hessian correction (``EngineConfig.hessian_correction``,
``ops.kernels.hessian``), with the VALU record loop and on the matrix cores.

Each configuration is a child process under its own time limit; the first that
fails or runs out of time ends the script (nothing more is started on the
device).  One JSON line per record, also appended to ``--record``
(``profiles/hessian_kernels.jsonl``).

The child builds the first date of ``bench.py``'s workload (seeded sources,
emulators and prior; the prior as the state: tip7 two 4-input bands, prosail10
ten 10-input bands, T = 500) at ``--size``^2 pixels, warms both kernels up, then
times ``K.hessian(gp="valu")`` and ``K.hessian(gp="mfma")`` alternating, with
device events: median, minimum and maximum of ``--reps`` calls each.  It also
runs each kernel once on a copy of the same precision rows and records the
largest difference of the two results, of the largest entry of the correction.

    python scripts/bench_hessian.py --configs tip7 prosail10 --size 10980
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one_config(config, size, reps):
    import numpy as np
    import torch

    import bench
    from kafka_inferenceengine_amd.ops import kernels as K
    from kafka_inferenceengine_amd.parallel import Comm, StripPartition

    if not torch.cuda.is_available():
        raise SystemExit("bench_hessian needs a GPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    a = argparse.Namespace(warmup=0, steps=1, resident=True, set=[], output=None, n_train=None, pool=1, cloud=0.2,
                           metrics=None, band_parallel=1, no_telemetry=True)
    mask = np.ones((size, size), dtype=bool)
    obs, kf, state, dates = bench.build(config, a, mask, StripPartition(mask, 0, 1), dev, Comm.single(dev))
    bands = kf._device_bands(dates[0])
    specs = [s for s, _ in bands]
    table = kf._band_table(bands, specs, [d for _, d in bands])
    n, N = kf.n_params, kf.N
    st = kf._materialize(state)
    if not K.hessian_mfma_supported(n, table, dev):
        raise SystemExit(f"{config}: {K.hessian_mfma_unsupported(n, table, dev)}")
    work = st.P.clone()
    plans, ms = {}, {"valu": [], "mfma": []}
    for gp in ms:
        K.hessian(n, table, st.x, work, N=N, gp=gp)          # warm-up of this shape
        plans[gp] = K.LAST_HESSIAN_PLAN["name"]
    torch.cuda.synchronize()
    for _ in range(reps):
        for gp in ms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            K.hessian(n, table, st.x, work, N=N, gp=gp)
            e1.record()
            e1.synchronize()
            ms[gp].append(e0.elapsed_time(e1))
    res = {}
    for gp in ms:
        work.copy_(st.P)
        K.hessian(n, table, st.x, work, N=N, gp=gp)
        res[gp] = work.clone()
    corr = float((res["valu"] - st.P).abs().max().item())
    diff = float((res["valu"] - res["mfma"]).abs().max().item())
    rec = {"bench": "kernel", "kernel": "hessian", "config": config, "size": size, "pixels": N, "n_params": n,
           "n_bands": len(bands), "n_train": int(specs[0].records.shape[0] * 2), "reps": reps, "plans": plans,
           "finite": bool(torch.isfinite(res["mfma"]).all().item()),
           "max_diff_of_largest_correction": diff / corr if corr > 0 else None, "largest_correction": corr}
    for gp, v in ms.items():
        rec[f"{gp}_ms_median"], rec[f"{gp}_ms_min"], rec[f"{gp}_ms_max"] = \
            round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)
    rec["valu_over_mfma"] = round(rec["valu_ms_median"] / rec["mfma_ms_median"], 3)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", nargs="+", default=["tip7", "prosail10"], choices=["tip7", "prosail10"])
    ap.add_argument("--size", type=int, default=10980, help="tile side")
    ap.add_argument("--reps", type=int, default=7, help="timed calls per kernel (>= 7)")
    ap.add_argument("--limit", type=int, default=500, help="seconds each configuration may take")
    ap.add_argument("--record", default=os.path.join(ROOT, "profiles", "hessian_kernels.jsonl"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 7:
        ap.error("--reps: at least 7")
    if a.child:
        return one_config(a.child, a.size, a.reps)
    for config in a.configs:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", config, "--size", str(a.size), "--reps",
               str(a.reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit, cwd=ROOT,
                               env=dict(os.environ, PYTHONPATH=ROOT))
        except subprocess.TimeoutExpired:
            raise SystemExit(f"{config}: no result within {a.limit} s; stopping")
        if r.returncode != 0:
            raise SystemExit(f"{config}: exit status {r.returncode}; stopping\n{r.stderr[-3000:]}")
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        if a.record:
            with open(a.record, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
