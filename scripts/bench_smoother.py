#!/usr/bin/env python
"""Cost of the fixed-interval (RTS) smoother (``LinearKalman.smooth``).

Two measurements, each GPU step a child process under its own time limit; the
first step that fails or runs out of time ends the script (nothing more is
started on the device).  One JSON line per record, also appended to ``--record``.

``kernels``: device-event times (median of ``--reps`` calls after warm-up) of
``smooth_kernel`` for n = 7 with mask {6} (the LAI propagator) and n = 10 with
the full mask, both kinds of the filtered rows, with the bytes per pixel it
moves (reads 2 (n + ntri) floats, writes n + ntri floats and the status byte)
and the effective bandwidth.  As the yardsticks on the same box: a plain device
copy of the same byte volume (half of it read, half written), and
``marginal_kernel`` (precision kind, with the mean) on the same N.

    python scripts/bench_smoother.py kernels --sizes 3882 10980

``e2e``: ``cli run --sensor bhr --size S S --steps K --out DIR --out-fast
--out-encoder device --smooth-out DIR2`` with the checkpoints on local disk:
the wall time of ``smooth()`` per step, split into checkpoint read, host-to-
device copy, kernel and output.

    python scripts/bench_smoother.py e2e --size 3882
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

CASES = {7: 1 << 6, 10: (1 << 10) - 1}     # n -> prop_mask


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
    """Child: times smooth / copy / marginal on one [size x size] state of n parameters."""
    import torch

    from kafka_inferenceengine_amd.ops import kernels as K

    if not torch.cuda.is_available():
        raise SystemExit("bench_smoother kernels needs a GPU")
    dev = torch.device("cuda")
    N = size * size
    nt = K.ntri(n)
    g = torch.Generator(device=dev).manual_seed(0)
    diag = {K.ntri(n) - K.ntri(n - j) for j in range(n)}

    def spd_rows(lo):
        # SPD by diagonal dominance: |off-diagonal| <= 0.05, diagonal in [lo, lo + 1)
        p = torch.empty((nt, N), device=dev)
        for t in range(nt):
            row = torch.rand(N, device=dev, generator=g)
            p[t] = row + lo if t in diag else 0.1 * row - 0.05
        return p

    x_a = torch.rand((n, N), device=dev, generator=g)
    x_next = torch.rand((n, N), device=dev, generator=g)
    p_a, p_next = spd_rows(1.0), spd_rows(1.0)
    x_out, p_out = torch.empty_like(x_a), torch.empty_like(p_a)
    status = torch.empty(N, dtype=torch.uint8, device=dev)
    m, q = [1.0] * n, [0.04] * n

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

    rd, wr = 8 * (n + nt), 4 * (n + nt) + 1
    out = []

    def rec(name, med, lo, hi, rd, wr, **kw):
        out.append({"bench": "kernel", "kernel": name, "size": size, "n_params": n, "ms_median": round(med, 4),
                    "ms_min": round(lo, 4), "ms_max": round(hi, 4), "reps": reps, "read_B_per_px": rd,
                    "write_B_per_px": wr, "GB_per_s": round((rd + wr) * N / (med * 1e-3) / 1e9, 1), **kw})

    for kind in ("precision", "covariance"):
        med, lo, hi = timed(lambda: K.smooth(n, x_a, p_a, x_next, p_next, x_out, p_out, status, kind=kind,
                                             prop_mask=CASES[n], m=m, q=q))
        fb = int(status.count_nonzero().item())
        assert fb == 0 and bool(torch.isfinite(p_out[:, ::4097]).all())
        rec(f"smooth_kernel/{kind}", med, lo, hi, rd, wr, prop_mask=CASES[n], fallback_pixels=fb)
    # a plain device copy of the same byte volume: 1.5 (n + nt) floats per pixel read and as many written
    del x_next, p_next, x_out, p_out
    half = (3 * (n + nt) * N) // 2
    src = torch.rand(half, device=dev, generator=g)
    dst = torch.empty_like(src)
    med, lo, hi = timed(lambda: dst.copy_(src))
    rec("device_copy", med, lo, hi, 6 * (n + nt), 6 * (n + nt))
    del src, dst
    mean, unc = torch.empty_like(x_a), torch.empty_like(x_a)
    med, lo, hi = timed(lambda: K.marginal(n, x_a, p_a, mean, unc, kind="precision"))
    rec("marginal_kernel/precision", med, lo, hi, 4 * (nt + n), 8 * n)
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
    folder = tempfile.mkdtemp(prefix="smoother_e2e_", dir=a.tmp)
    try:
        out = child([sys.executable, "-m", "kafka_inferenceengine_amd", "run", "--sensor", "bhr", "--size",
                     str(a.size), str(a.size), "--steps", str(a.steps), "--out", os.path.join(folder, "filtered"),
                     "--out-fast", "--out-encoder", "device", "--smooth-out", os.path.join(folder, "smoothed")],
                    a.limit, "e2e")
    finally:
        shutil.rmtree(folder, ignore_errors=True)
    rec = json.loads(out.strip().splitlines()[-1])
    s = rec["smooth"]
    k = len(s["timesteps"])
    emit({"bench": "e2e", "size": a.size, "steps": k, "forward_wall_s": rec["wall_s"], "smooth_wall_s": s["wall_s"],
          "smooth_per_step_ms": round(1e3 * s["wall_s"] / max(k, 1), 1), "read_ms": s["read_s"], "h2d_ms": s["h2d_s"],
          "kernel_ms": s["kernel_s"], "output_ms": s["output_s"], "fallback_pixels": s["fallback_pixels"],
          "checkpoint_GB": rec.get("checkpoint", {}).get("GB")}, a.record)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernels", "e2e", "_kernel_child"])
    ap.add_argument("--sizes", type=int, nargs="+", default=[3882, 10980])
    ap.add_argument("--n", type=int, nargs="+", default=[7, 10], choices=sorted(CASES))
    ap.add_argument("--reps", type=int, default=7, help="timed calls per kernel (>= 5)")
    ap.add_argument("--size", type=int, default=3882, help="e2e: the tile's side")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--limit", type=int, default=240, help="seconds each GPU step may take")
    ap.add_argument("--tmp", default=None, help="e2e: where the checkpoints and GeoTIFF folders are made (and removed)")
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
