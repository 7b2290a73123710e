"""Time of the GP predictive-variance kernels (csrc/kf_gp_variance.hip) for the JRC-TIP bands
on one tile: ``python scripts/bench_gp_variance.py [--mode variance] [--side 1024] [--n-train 500]
[--reps 30]``.  Device events around each launch pair (both bands), after a warm-up; prints one JSON
line with the median, the spread and the table sizes.  Needs a GPU.

``--mode variance``: ``gp_variance_kernel``, one launch per band.  ``weight``: ``gp_obs_weight_kernel``,
both bands in one launch, every pixel observed (DN16).  ``weight_half``: the same with every other
64-pixel tile without an observation.  ``date``: a JRC-TIP engine run of ``--dates`` dates on the tile
with ``emulator_uncertainty='inflate'``; prints the device time of every phase per date, the
inflation launch ('inflate') next to the date's analysis launches."""
import argparse
import datetime as dt
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import kafka_inferenceengine_amd as k  # noqa: E402
from kafka_inferenceengine_amd.engine.bands import DeviceBand  # noqa: E402
from kafka_inferenceengine_amd.ops import kernels as K  # noqa: E402


def date_phases(a, dev):
    """Device ms per date of every engine phase, with the inflation on."""
    mask = np.ones((a.side, a.side), bool)
    dates = [dt.datetime(2017, 1, 1) + dt.timedelta(days=16 * i) for i in range(a.dates + 1)]
    obs = k.SyntheticBHRObservations(mask, dates=dates, n_train=a.n_train, device=dev, n_pool=4, stream=False, seed=0)
    kf = k.LinearKalman(obs, None, mask, k.create_nonlinear_observation_operator, k.TIP_PARAMETERS,
                        state_propagation=k.propagate_information_filter_LAI, device=dev,
                        config=k.EngineConfig(emulator_uncertainty="inflate", phase_timing=True))
    kf.set_trajectory_model()
    kf.set_trajectory_uncertainty(np.array([0, 0, 0, 0, 0, 0, 0.04]))
    x0, Pinv = k.JRCPrior(k.TIP_PARAMETERS, mask).process_prior(None)
    kf.run(dates[:2], x0, None, Pinv)           # warm-up: one date
    torch.cuda.synchronize()
    kf.timer.snapshot()
    kf.timer.run_totals.clear()
    seen = len(kf.metrics.records)
    kf.run(dates, x0, None, Pinv)
    torch.cuda.synchronize()
    kf.timer.snapshot()
    recs = [r for r in kf.metrics.records[seen:] if r.get("event") == "date"]
    print(json.dumps({"bench": "gp_obs_weight_date", "side": a.side, "n_train": a.n_train, "dates": len(recs),
                      "gn_iterations": [r["n_iter"] for r in recs], "weight_ratio": recs[-1]["emulator"],
                      "ms_per_date": {n: round(v / len(recs), 4) for n, v in sorted(kf.timer.run_totals.items())}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("variance", "weight", "weight_half", "date"), default="variance")
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--n-train", type=int, default=500)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dates", type=int, default=8)
    ap.add_argument("--grid", type=int, default=0, help="workgroups per band (0: the launcher's default)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gp_variance needs a GPU")
    dev = torch.device("cuda")
    if a.mode == "date":
        return date_phases(a, dev)
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

    if a.mode != "variance":
        # DN16 reflectances of 0.05 .. 0.5; weight_half: every other 64-pixel tile all nodata
        dn = rng.integers(500, 5000, size=(2, N)).astype(np.int16)
        if a.mode == "weight_half":
            dn[:, (np.arange(N) // 64) % 2 == 1] = 0
        dnd = torch.from_numpy(dn).to(dev)
        dbs = [DeviceBand(K.OBS_DN16, dn=dnd[b], scale=1e-4, rel_unc=0.05, unc_floor=0.004) for b in range(2)]
        yw = torch.empty((2, 2, N), device=dev)

        def launch():  # noqa: F811
            K.gp_variance(7, specs, xd, list(out), N=N, obs=dbs, y_out=list(yw[0]), w_out=list(yw[1]),
                          grid=a.grid)

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
    flop = 2.0 * 3 * (nch * (nch + 1) // 2) * 32 * 32 * N * len(ems) * (0.5 if a.mode == "weight_half" else 1.0)
    res = {
        "bench": "gp_variance", "mode": a.mode, "side": a.side, "pixels": N, "bands": len(ems), "n_train": a.n_train,
        "grid": a.grid, "ms_median": float(np.median(ms)), "ms_min": float(ms[0]), "ms_max": float(ms[-1]),
        "ms_p10": float(ms[len(ms) // 10]), "ms_p90": float(ms[-1 - len(ms) // 10]), "reps": a.reps,
        "table_bytes_per_band": int(sum(t.numel() * t.element_size() for t in fields[0][:2])),
        "lds_bytes": nch * 8192 + 2048, "tflops_split_products": flop / (np.median(ms) * 1e-3) / 1e12,
        "finite": bool(torch.isfinite(out).all()), "std_mean": float(out.clamp(min=0).sqrt().mean())}
    if a.mode != "variance":
        res["observed"] = float((yw[1] > 0).float().mean())
        res["weight_ratio"] = float((1.0 - yw[1] * out)[yw[1] > 0].mean())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
