#!/usr/bin/env python
"""Cost of K2, the split path's GP operator pass (``ops.kernels.gp_operator``), with the VALU
record loop and on the matrix cores (csrc/kf_gp_operator_mfma.hip).

Each configuration is a child process under its own time limit; the first that fails or runs
out of time ends the script (nothing more is started on the device).  One JSON line per
record, also appended to ``--record`` (``profiles/gp_operator_kernels.jsonl``).

Kernel configurations ``n,d,bands,T``: synthetic emulators (models/gp.py make_prosail_emulators
for 10 inputs, make_tip_emulators for 4, one seed per band pair) on the JRC-TIP state maps
(d = 4) or the whole state (d = 10), float32 observations with every fifth run of 4096 pixels
under cloud (both kernels skip a wave no lane of which observes), the state drawn from the
training inputs, ``--size``^2 pixels.  The child warms both kernels up, then times
``K.gp_operator(gp="valu")`` and ``gp="mfma"`` alternating with device events (median, minimum
and maximum of ``--reps`` calls each) and records the largest difference of the two results.  ``--f64`` adds ``gp="f64"``
(csrc/kf_gp_operator_f64.hip) as a third alternating arm, with its ratio to the matrix-core kernel.

``engine:CONFIG``: ``bench.py --config CONFIG --set gp_split=always --set convergence_chunk=tile``
(the per-chunk exit test keeps a date fused) under ``--set split_gp=valu`` and ``--set split_gp=mfma``, a fresh process per run, the two settings alternating twice,
``--steps`` timed dates after two warm-up dates; ms per step of each run as bench.py reports it.

    python scripts/bench_gp_operator.py --size 4096
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

KERNEL_CONFIGS = ["10,10,10,250", "7,4,2,500", "10,4,4,500", "7,4,8,500"]


def stats(rec, key, v):
    rec[f"{key}_ms_median"], rec[f"{key}_ms_min"], rec[f"{key}_ms_max"] = \
        round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)


def kernel_config(config, size, reps, f64=False):
    import numpy as np
    import torch

    import kafka_inferenceengine_amd as k
    from kafka_inferenceengine_amd.engine.bands import DeviceBand, RecordCache, build_table
    from kafka_inferenceengine_amd.ops import kernels as K

    if not torch.cuda.is_available():
        raise SystemExit("bench_gp_operator needs a GPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    n, d, nb, T = (int(v) for v in config.split(","))
    N = size * size
    rng = np.random.default_rng(0)
    if d == 10:
        ems = k.make_prosail_emulators(n_bands=nb, n_train=T)
        maps = [list(range(10))] * nb
    else:
        ems = [em for s in range((nb + 1) // 2) for em in k.make_tip_emulators(n_train=T, seed=s)][:nb]
        maps = [list(k.TIP_BAND_MAPPER[b % 2]) for b in range(nb)]
    specs = [k.gp_spec(em, mp) for em, mp in zip(ems, maps)]
    x = rng.uniform(0.2, 0.8, (n, N)).astype(np.float32)
    for em, mp in zip(ems[:2], maps[:2]):   # training inputs, jittered: every band is evaluated inside its box
        x[mp] = (em.inputs[rng.integers(0, em.inputs.shape[0], N)] * rng.uniform(0.98, 1.02, (N, d))).T
    w = np.where((np.arange(N) // 4096) % 5 == 0, 0.0, 1e4).astype(np.float32)
    y, w = torch.full((N,), 0.3, device=dev), torch.from_numpy(w).to(dev)
    table = build_table(specs, [DeviceBand(K.OBS_F32, y=y, w=w) for _ in specs], n, RecordCache(), dev)
    why = K.gp_operator_mfma_unsupported(n, table, dev)
    if why is not None:
        raise SystemExit(f"{config}: {why}")
    xd = torch.from_numpy(x).to(dev)
    h0, h = torch.empty((nb, N), device=dev), torch.empty((nb * n, N), device=dev)
    ms, out = {"valu": [], "mfma": []}, {}
    if f64:                                  # the float64 kernel (csrc/kf_gp_operator_f64.hip) as a third arm
        why = K.gp_operator_f64_unsupported(n, table, dev)
        if why is not None:
            raise SystemExit(f"{config}: {why}")
        ms["f64"] = []
    for gp in ms:                            # warm-up of this shape, and the results to compare
        K.gp_operator(n, table, xd, h0, h, N=N, d=d, gp=gp)
        out[gp] = (h0.clone(), h.clone())
        if gp == "mfma":
            plan = K.LAST_GP_OPERATOR_PLAN
    torch.cuda.synchronize()
    for _ in range(reps):
        for gp in ms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            K.gp_operator(n, table, xd, h0, h, N=N, d=d, gp=gp)
            e1.record()
            e1.synchronize()
            ms[gp].append(e0.elapsed_time(e1))
    rec = {"bench": "kernel", "kernel": "gp_operator", "config": config, "size": size, "pixels": N, "n_params": n,
           "d": d, "n_bands": nb, "n_train": T, "reps": reps, "names": list(plan["names"]),
           "resident": list(plan["resident"]), "finite": bool(torch.isfinite(out["mfma"][1]).all().item()),
           "max_diff_value": float((out["valu"][0] - out["mfma"][0]).abs().max().item()),
           "max_diff_gradient": float((out["valu"][1] - out["mfma"][1]).abs().max().item())}
    for gp, v in ms.items():
        stats(rec, gp, v)
    rec["valu_over_mfma"] = round(rec["valu_ms_median"] / rec["mfma_ms_median"], 3)
    if f64:
        rec["f64_over_mfma"] = round(rec["f64_ms_median"] / rec["mfma_ms_median"], 3)
        rec["max_diff_value_f64_mfma"] = float((out["f64"][0] - out["mfma"][0]).abs().max().item())
        rec["max_diff_gradient_f64_mfma"] = float((out["f64"][1] - out["mfma"][1]).abs().max().item())
    print(json.dumps(rec))


def engine_config(config, size, steps, limit):
    """bench.py itself, a fresh process per run, the two settings alternating twice."""
    ms = {"valu": [], "mfma": []}
    for _ in range(2):
        for gp in ms:
            cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", config, "--size", str(size),
                   "--steps", str(steps), "--warmup", "2", "--set", "gp_split=always", "--set", "convergence_chunk=tile",
                   "--set", f"split_gp={gp}"]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, cwd=ROOT)
            if r.returncode != 0:
                raise SystemExit(f"bench.py split_gp={gp}: exit status {r.returncode}\n{r.stderr[-3000:]}")
            ms[gp].append(json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"])
    rec = {"bench": "engine", "config": config, "size": size, "pixels": size * size, "gp_split": "always",
           "convergence_chunk": "tile", "steps": steps, "valu_ms_per_step": ms["valu"], "mfma_ms_per_step": ms["mfma"]}
    rec["valu_over_mfma"] = round(min(ms["valu"]) / min(ms["mfma"]), 3)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", nargs="+", default=KERNEL_CONFIGS + ["engine:prosail10"])
    ap.add_argument("--size", type=int, default=4096, help="tile side")
    ap.add_argument("--reps", type=int, default=9, help="timed calls per kernel (>= 7)")
    ap.add_argument("--steps", type=int, default=4, help="dates of an engine run")
    ap.add_argument("--limit", type=int, default=400, help="seconds each configuration may take")
    ap.add_argument("--record", default=os.path.join(ROOT, "profiles", "gp_operator_kernels.jsonl"))
    ap.add_argument("--f64", action="store_true", help="kernel configurations: time gp='f64' as a third arm")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 7:
        ap.error("--reps: at least 7")
    if a.child:
        if a.child.startswith("engine:"):
            return engine_config(a.child.split(":", 1)[1], a.size, a.steps, a.limit)
        return kernel_config(a.child, a.size, a.reps, a.f64)
    for config in a.configs:
        engine = config.startswith("engine:")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", config, "--size", str(a.size), "--reps",
               str(a.reps), "--steps", str(a.steps)] + (["--f64"] if a.f64 else [])
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=(5 if engine else 1) * a.limit, cwd=ROOT,
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
