#!/usr/bin/env python
"""Cost of the innovation statistics and the chi-square gate
(``EngineConfig.innovation_gate`` / ``innovation_stats``, ``ops.kernels.innovation``).

Two measurements, each GPU step a child process under its own time limit; the
first step that fails or runs out of time ends the script (nothing more is
started on the device).  One JSON line per record, also appended to ``--record``.

``kernels``: device-event times (median of ``--reps`` calls after warm-up) of
``innovation_kernel`` alone on the first date of ``bench.py``'s tip7 and
prosail10 workloads (the sources, emulators and prior of the benchmark, the
prior as the state): statistics only, and with a gate writing the screened
planes.  The kernel evaluates the GP bands with the VALU record loop.
``joint``: the joint instantiation (``innovation_joint_kernel``: the statistics
plus d2 = r^T S^-1 r and log det S); ``joint_kept``: the second launch of a
gated date under ``innovation_evidence`` (gate 0 on the screened bands, writing
status, nobs, d2 and logdet only).

    python scripts/bench_innovation.py kernels --configs tip7 prosail10 --size 10980

``e2e``: ``bench.py --config C`` four ways -- default, ``--set
fuse_propagation=false`` (the unfused path a screened date also takes), ``--set
innovation_stats=true`` and ``--set innovation_gate=K`` -- ``--rounds`` times in
that order, with the ms/step of every run and the ratios of the means.

    python scripts/bench_innovation.py e2e --configs tip7 prosail10
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

VARIANTS = (("default", []), ("unfused", ["--set", "fuse_propagation=false"]),
            ("stats", ["--set", "innovation_stats=true"]), ("gated", None))


def emit(rec, record):
    line = json.dumps(rec)
    print(line, flush=True)
    if record:
        with open(record, "a") as f:
            f.write(line + "\n")


def child(cmd, limit, what):
    """One GPU step: its own process, its own time limit.  -> stdout, or exits."""
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, cwd=ROOT,
                           env=dict(os.environ, PYTHONPATH=ROOT))
    except subprocess.TimeoutExpired:
        raise SystemExit(f"{what}: no result within {limit} s; stopping")
    if r.returncode != 0:
        raise SystemExit(f"{what}: exit status {r.returncode}; stopping\n{r.stderr[-3000:]}")
    return r.stdout


# ------------------------------------------------------------------ kernels
def one_kernel_config(config, size, reps, gate, device=None):
    """Child: times innovation_kernel on the first date of one bench.py workload
    (``device="cpu"``: the host runner, wall-clock times -- a dry run of the script)."""
    import time

    import numpy as np
    import torch

    import bench
    from kafka_inferenceengine_amd.ops import kernels as K
    from kafka_inferenceengine_amd.parallel import Comm, StripPartition

    if device != "cpu" and not torch.cuda.is_available():
        raise SystemExit("bench_innovation kernels needs a GPU (--device cpu: a dry run on the host runner)")
    dev = torch.device("cpu") if device == "cpu" else torch.device("cuda", torch.cuda.current_device())
    a = argparse.Namespace(warmup=0, steps=1, resident=True, set=[], output=None, n_train=None, pool=1, cloud=0.2,
                           metrics=None, band_parallel=1, no_telemetry=True)
    mask = np.ones((size, size), dtype=bool)
    comm = Comm.single(dev)
    obs, kf, state, dates = bench.build(config, a, mask, StripPartition(mask, 0, 1), dev, comm)
    bands = kf._device_bands(dates[0])
    specs = [s for s, _ in bands]
    table = kf._band_table(bands, specs, [d for _, d in bands])
    groups = kf._band_groups(dates[0], len(specs))
    n, N = kf.n_params, kf.N
    st = kf._materialize(state)
    chi2 = torch.empty(N, dtype=torch.float32, device=dev)
    nobs, nrej, status = (torch.empty(N, dtype=torch.uint8, device=dev) for _ in range(3))
    screened = [torch.empty_like(getattr(db, kf._nodata_plane(db))) for _, db in bands]

    def timed(fn):
        for _ in range(2):
            fn()
        ms = []
        if dev.type != "cuda":
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                ms.append(1e3 * (time.perf_counter() - t0))
            return statistics.median(ms), min(ms), max(ms)
        torch.cuda.synchronize()
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms), max(ms)

    import dataclasses
    d2, logdet = (torch.empty(N, dtype=torch.float32, device=dev) for _ in range(2))
    # the screened bands of the gated launch: what the second launch of a gated date reads
    kept = [(s, dataclasses.replace(db, **{kf._nodata_plane(db): t})) for (s, db), t in zip(bands, screened)]
    out = []
    for name, kw in (("stats", dict(gate=0.0)), ("gated", dict(gate=gate, screened=screened)),
                     ("joint", dict(gate=0.0, d2=d2, logdet=logdet)), ("joint_kept", None)):
        if kw is None:
            table2 = kf._innovation_table(specs, kept)
            kw = dict(gate=0.0)
            med, lo, hi = timed(lambda: K.innovation(n, table2, st.x, st.P, kind=st.kind, N=N, nobs=nobs,
                                                     status=status, d2=d2, logdet=logdet))
        else:
            med, lo, hi = timed(lambda: K.innovation(n, table, st.x, st.P, kind=st.kind, N=N, chi2=chi2, nobs=nobs,
                                                     nrej=nrej, status=status, groups=groups, **kw))
        seen = int(nobs.sum(dtype=torch.int64).item())
        fin = torch.isfinite(d2)
        joint = {} if name in ("stats", "gated") else {
            "d2_per_obs": round(float(torch.where(fin, d2, torch.zeros_like(d2)).sum(dtype=torch.float64).item())
                                / max(seen, 1), 4), "joint_nan": int((~fin).sum().item())}
        out.append({"bench": "kernel", "kernel": f"innovation_kernel/{name}", **joint, "config": config, "size": size,
                    "device": dev.type, "n_params": n, "n_bands": len(bands), "kind": st.kind, "gate": kw["gate"],
                    "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "reps": reps,
                    "observed_bands": seen, "rejected_bands": int(nrej.sum(dtype=torch.int64).item()),
                    "unscreenable": int(status.count_nonzero().item()),
                    "chi2_per_obs": round(float(chi2.sum(dtype=torch.float64).item()) / max(seen, 1), 4),
                    "px_per_s": round(N / (med * 1e-3), 1)})
    print(json.dumps(out))


def kernels(a):
    for config in a.configs:
        out = child([sys.executable, os.path.abspath(__file__), "_kernel_child", "--configs", config, "--size",
                     str(a.size), "--reps", str(a.reps), "--gate", str(a.gate)] +
                    (["--device", a.device] if a.device else []), a.limit,
                    f"kernels {config} {a.size}^2")
        for rec in json.loads(out.strip().splitlines()[-1]):
            emit(rec, a.record)


# --------------------------------------------------------------------- e2e
def e2e(a):
    for config in a.configs:
        runs = {name: [] for name, _ in VARIANTS}
        for _ in range(a.rounds):
            for name, extra in VARIANTS:
                extra = ["--set", f"innovation_gate={a.gate}"] if extra is None else extra
                cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", config, "--steps",
                       str(a.steps), "--warmup", str(a.warmup), "--no-telemetry"] + extra
                if a.size:
                    cmd += ["--size", str(a.size)]
                rec = json.loads(child(cmd, a.limit, f"e2e {config} {name}").strip().splitlines()[-1])
                runs[name].append(rec["ms_per_step"])
                if not rec["config"]["finite"]:
                    raise SystemExit(f"e2e {config} {name}: state not finite; stopping")
        mean = {name: statistics.fmean(v) for name, v in runs.items()}
        emit({"bench": "e2e", "config": config, "size": a.size, "steps": a.steps, "warmup": a.warmup, "gate": a.gate,
              "ms_per_step": runs, "mean_ms_per_step": {name: round(v, 3) for name, v in mean.items()},
              "gated_over_default": round(mean["gated"] / mean["default"], 3),
              "gated_over_unfused": round(mean["gated"] / mean["unfused"], 3),
              "stats_over_unfused": round(mean["stats"] / mean["unfused"], 3)}, a.record)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernels", "e2e", "_kernel_child"])
    ap.add_argument("--configs", nargs="+", default=["tip7", "prosail10"], choices=["tip7", "prosail10"])
    ap.add_argument("--size", type=int, default=None, help="tile side (default: 10980 for kernels, bench.py's for e2e)")
    ap.add_argument("--reps", type=int, default=7, help="timed calls per kernel (>= 5)")
    ap.add_argument("--gate", type=float, default=4.0)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2, help="e2e: times the four runs are repeated")
    ap.add_argument("--limit", type=int, default=300, help="seconds each GPU step may take")
    ap.add_argument("--device", default=None, choices=["cpu"], help="kernels: dry run on the host runner")
    ap.add_argument("--record", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least 5")
    if a.what == "_kernel_child":
        one_kernel_config(a.configs[0], a.size or 10980, a.reps, a.gate, a.device)
    elif a.what == "kernels":
        a.size = a.size or 10980
        kernels(a)
    else:
        e2e(a)


if __name__ == "__main__":
    main()
