#!/usr/bin/env python
"""Cost of the marginal uncertainty rasters (``uncertainty="marginal"``).

Two measurements, each GPU step a child process under its own time limit; the
first step that fails or runs out of time ends the script (nothing more is
started on the device).  One JSON line per record, also appended to ``--record``.

``kernels``: device-event times (median of ``--reps`` calls after warm-up) of
``marginal_kernel`` for both kinds and, as the yardstick, ``unpack_kernel`` on
the same tensors, with the bytes per pixel each moves and the effective
bandwidth.  Precision kind: reads 4 (ntri + n) B/px with the mean (4 ntri
without), covariance kind and unpack: 4 (n + n) (4 n without); all write 8 n
(4 n without the mean).

    python scripts/bench_marginal.py kernels --sizes 3882 10980 --n 7 10

``e2e``: ``cli run --sensor bhr --size S S --steps 5 --out DIR --out-fast
--out-encoder device`` in three modes -- the default (fused conditional
rasters), ``--no-fuse-output`` (the existing dump pass) and ``--out-unc
marginal`` -- alternated, ``--rounds`` times each.  Per mode: per-date wall
time ((dates 2.. + final drain) / (dates - 1)), the writer's ``write_ms`` and
the ``analysis`` / ``output`` phase times.  default -> no-fuse is the price of
the non-fused path, no-fuse -> marginal that of the new kernel.

    python scripts/bench_marginal.py e2e --size 10980 --rounds 2
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = {"default": [], "no_fuse_output": ["--no-fuse-output"], "marginal": ["--out-unc", "marginal"]}


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
def one_kernel_config(size, n, reps):
    """Child: times unpack / marginal on one [size x size] state of n parameters."""
    import torch

    from kafka_inferenceengine_amd.ops import kernels as K

    if not torch.cuda.is_available():
        raise SystemExit("bench_marginal kernels needs a GPU")
    dev = torch.device("cuda")
    N = size * size
    nt = K.ntri(n)
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand((n, N), device=dev, generator=g)
    # SPD by diagonal dominance: |off-diagonal| <= 0.05, diagonal in [1, 2); as a
    # covariance the same rows have a positive diagonal
    p = torch.empty((nt, N), device=dev)
    diag = {K.ntri(n) - K.ntri(n - j) for j in range(n)}
    for t in range(nt):
        row = torch.rand(N, device=dev, generator=g)
        p[t] = row + 1.0 if t in diag else 0.1 * row - 0.05
    mean = torch.empty((n, N), device=dev)
    unc = torch.empty((n, N), device=dev)

    def timed(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms), max(ms)

    out = []
    for with_mean in (True, False):
        m = mean if with_mean else None
        wr = 4 * n * (2 if with_mean else 1)
        cases = (("unpack_kernel", 4 * n * (2 if with_mean else 1), lambda: K.unpack(n, x, p, m, unc)),
                 ("marginal_kernel/precision", 4 * (nt + (n if with_mean else 0)),
                  lambda: K.marginal(n, x, p, m, unc, kind="precision")),
                 ("marginal_kernel/covariance", 4 * n * (2 if with_mean else 1),
                  lambda: K.marginal(n, x, p, m, unc, kind="covariance")))
        for name, rd, fn in cases:
            med, lo, hi = timed(fn)
            assert bool(torch.isfinite(unc[:, ::4097]).all())
            out.append({"bench": "kernel", "kernel": name, "size": size, "n_params": n, "mean": with_mean,
                        "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "reps": reps,
                        "read_B_per_px": rd, "write_B_per_px": wr,
                        "GB_per_s": round((rd + wr) * N / (med * 1e-3) / 1e9, 1)})
    print(json.dumps(out))


def kernels(a):
    for size in a.sizes:
        for n in a.n:
            out = child([sys.executable, os.path.abspath(__file__), "_kernel_child", "--sizes", str(size), "--n", str(n),
                         "--reps", str(a.reps)], a.limit, f"kernels {size}^2 n={n}")
            for rec in json.loads(out.strip().splitlines()[-1]):
                emit(rec, a.record)


# --------------------------------------------------------------------- e2e
def e2e(a):
    for rnd in range(a.rounds):
        for mode, flags in MODES.items():
            folder = tempfile.mkdtemp(prefix="marginal_e2e_", dir=a.tmp)
            try:
                out = child([sys.executable, "-m", "kafka_inferenceengine_amd", "run", "--sensor", "bhr", "--size",
                             str(a.size), str(a.size), "--steps", str(a.steps), "--out", folder, "--out-fast",
                             "--out-encoder", "device", "--out-keep", "2", "--phase-timing", *flags],
                            a.limit, f"e2e {mode} round {rnd + 1}")
            finally:
                shutil.rmtree(folder, ignore_errors=True)
            rec = json.loads(out.strip().splitlines()[-1])
            walls = rec["timestep_wall_ms"]
            o = rec.get("output", {})
            ph = rec.get("phases_ms", {})
            emit({"bench": "e2e", "mode": mode, "round": rnd + 1, "size": a.size, "dates": len(walls),
                  "per_date_ms": round((sum(walls[1:]) + 1e3 * rec["output_drain_s"]) / max(len(walls) - 1, 1), 1),
                  "timestep_wall_ms": walls, "output_drain_s": rec["output_drain_s"], "wall_s": rec["wall_s"],
                  "write_ms": o.get("write_ms"), "uncertainty": o.get("uncertainty"),
                  "file_bytes": o.get("file_bytes"),
                  "phases_ms": ph}, a.record)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernels", "e2e", "_kernel_child"])
    ap.add_argument("--sizes", type=int, nargs="+", default=[3882, 10980])
    ap.add_argument("--n", type=int, nargs="+", default=[7, 10])
    ap.add_argument("--reps", type=int, default=7, help="timed calls per kernel (>= 5)")
    ap.add_argument("--size", type=int, default=10980, help="e2e: the tile's side")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds each GPU step may take")
    ap.add_argument("--tmp", default=None, help="e2e: where the GeoTIFF folders are made (and removed)")
    ap.add_argument("--record", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least 5")
    if a.what == "_kernel_child":
        one_kernel_config(a.sizes[0], a.n[0], a.reps)
    elif a.what == "kernels":
        kernels(a)
    else:
        e2e(a)


if __name__ == "__main__":
    main()
