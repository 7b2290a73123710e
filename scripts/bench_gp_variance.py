"""Time of the GP predictive-variance kernel (csrc/kf_gp_variance.hip) for the JRC-TIP bands
on one tile: ``python scripts/bench_gp_variance.py [--side 1024] [--n-train 500] [--reps 30]``.
Device events around each launch pair (both bands), after a warm-up; prints one JSON line with
the median, the spread and the table sizes.  Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import kafka_inferenceengine_amd as k  # noqa: E402
from kafka_inferenceengine_amd.ops import kernels as K  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--n-train", type=int, default=500)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gp_variance needs a GPU")
    dev = torch.device("cuda")
    N = a.side * a.side
    ems = k.make_tip_emulators(n_train=a.n_train)
    specs = [k.gp_spec(em, list(m)) for em, m in zip(ems, k.TIP_BAND_MAPPER)]
    mu, P, _ = k.tip_prior()
    rng = np.random.default_rng(0)
    x = (mu[:, None] + rng.normal(size=(7, N)) * np.sqrt(np.diag(P))[:, None] * 0.3).astype(np.float32)
    x[6] = np.clip(x[6], 0.05, 0.95)
    xd = torch.from_numpy(x).to(dev)
    out = torch.empty((2, N), device=dev)

    def launch():
        for b, sp in enumerate(specs):
            K.gp_variance(7, sp, xd, out[b], N=N)

    for _ in range(a.warmup):
        launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = np.sort(np.array(ms))
    fields = [K._gpv_fields(em, dev) for em in ems]
    nch = fields[0][2]
    # multiply-adds of the three split products over the blocks of the lower triangle
    flop = 2.0 * 3 * (nch * (nch + 1) // 2) * 32 * 32 * N * len(ems)
    print(json.dumps({
        "bench": "gp_variance", "side": a.side, "pixels": N, "bands": len(ems), "n_train": a.n_train,
        "ms_median": float(np.median(ms)), "ms_min": float(ms[0]), "ms_max": float(ms[-1]),
        "ms_p10": float(ms[len(ms) // 10]), "ms_p90": float(ms[-1 - len(ms) // 10]), "reps": a.reps,
        "table_bytes_per_band": int(sum(t.numel() * t.element_size() for t in fields[0][:2])),
        "lds_bytes": nch * 8192 + 2048, "tflops_split_products": flop / (np.median(ms) * 1e-3) / 1e12,
        "finite": bool(torch.isfinite(out).all()), "std_mean": float(out.clamp(min=0).sqrt().mean())}))


if __name__ == "__main__":
    main()
