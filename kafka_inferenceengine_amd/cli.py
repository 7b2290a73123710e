"""Command-line drivers (the reference's de-facto CLI are its three driver
scripts):

  run    — assimilation run: TIP/BHR (kafka_test.py), S2 PROSAIL (kafka_test_S2.py),
           S1 SAR, identity, multi-sensor; synthetic sensors or file readers;
           GeoTIFF or in-memory output; checkpoint/resume; metrics JSONL.
           Launch with torchrun for tile-DP over GPUs.
  farm   — chunk farming over ranks (kafka_test_Py36.py: get_chunks + client.map).
  chunks — print get_chunks(nx, ny, block).
  info   — device, native extension and compiled kernel sizes.

Examples:
  python -m kafka_inferenceengine_amd run --sensor bhr --size 2400 2400 --steps 23 --out /tmp/kafka
  torchrun --nproc-per-node 8 -m kafka_inferenceengine_amd run --sensor s2 --size 10980 10980
  python -m kafka_inferenceengine_amd run --sensor s2 --s2-folder DATA --emulator-folder EMUS --mask mask.tif
"""
from __future__ import annotations

import argparse
import datetime as dt
import json
import logging
import os
import sys

import numpy as np


def _mask(args):
    from .input_output.tiff import read_tiff, tiff_info

    if args.mask:
        m, info = read_tiff(args.mask)
        return m.astype(bool), info
    ref = _file_reference_raster(args)
    if ref is not None:                 # file-driven run: the grid of the data (ROI-cropped)
        info = tiff_info(ref)
        h, w = info["shape"]
        roi = getattr(args, "roi", None)
        if roi:
            h, w = roi[3] - roi[1], roi[2] - roi[0]
            gt = list(info.get("geotransform", [0, 1, 0, 0, 0, -1]))
            gt[0] += roi[0] * gt[1]
            gt[3] += roi[1] * gt[5]
            info["geotransform"] = gt
        return np.ones((h, w), dtype=bool), info
    h, w = args.size
    return np.ones((h, w), dtype=bool), {}


def _file_reference_raster(args):
    """First raster of a file-driven BHR / S2 / S1 run (defines the grid when no --mask)."""
    import glob
    import os

    if getattr(args, "bhr_folder", None):
        f = sorted(glob.glob(os.path.join(args.bhr_folder, "*_kernels_b0_k0.tif")))
    elif getattr(args, "s2_folder", None):
        f = sorted(glob.glob(os.path.join(args.s2_folder, "**", "B02_sur.tif"), recursive=True))
    elif getattr(args, "s1_folder", None):
        f = sorted(glob.glob(os.path.join(args.s1_folder, "S1_*", "theta.tif")))
    else:
        return None
    if not f:
        raise SystemExit("no input rasters found in the data folder")
    return f[0]


# The reference drivers' chunking: one LinearKalman per get_chunks tile, so the
# Gauss-Newton exit test is taken per chunk -- 256^2 for the MCD43 / TIP driver
# (kafka_test_Py36.py:241), 128^2 for the Sentinel-2 driver (kafka_test_S2.py:202)
DRIVER_CHUNK = {"bhr": 256, "identity": 256, "s2": 128, "multisensor": 128}


def _engine_config(args):
    """EngineConfig of a run: the command line / YAML, with the reference
    driver's per-chunk convergence as the default (``--convergence-chunk tile``
    tests over the whole state instead)."""
    from .engine.config import EngineConfig

    cfg = EngineConfig.from_args(args)
    if getattr(args, "evidence_out", None) or getattr(args, "scan_q", None):
        cfg.innovation_evidence = True
    if getattr(args, "smooth_out", None):
        # the backward pass reads every step's filtered state
        cfg.checkpoint_every, cfg.checkpoint_keep = 1, 0
        if not cfg.checkpoint_dir:
            cfg.checkpoint_dir = os.path.join(args.smooth_out, "checkpoints")
    explicit = getattr(args, "convergence_chunk", None) is not None
    if not explicit and getattr(args, "config_file", None):
        import yaml
        with open(args.config_file) as f:
            explicit = "convergence_chunk" in (yaml.safe_load(f) or {})
    if not explicit and cfg.convergence_chunk is None and args.sensor in DRIVER_CHUNK and cfg.spatial_gamma <= 0:
        b = DRIVER_CHUNK[args.sensor]
        cfg.convergence_chunk = [b, b]
        cfg.validate()
    return cfg


def _build(args, comm, q_scale=None):
    """The engine of a run.  ``q_scale`` (default ``--q-scale``) multiplies the
    sensor's built-in model error Q."""
    import kafka_inferenceengine_amd as k
    from .parallel import StripPartition

    mask, info = _mask(args)
    part = StripPartition(mask, comm.rank, comm.world)
    dev = comm.device
    cfg = _engine_config(args)
    syn = dict(partition=part, device=dev, stream=True, cloud_fraction=args.cloud, seed=args.seed)
    if args.sensor == "bhr":
        if args.bhr_folder:      # MCD43 kernel-weight rasters (kafka_test.py:156-217)
            from .input_output.sentinel import BHRObservations
            emu = args.emulator or k.make_tip_emulators(n_train=args.n_train or 500)
            roi = args.roi or [0, 0, None, None]
            obs = BHRObservations(emu, args.bhr_folder, period=args.period, ulx=roi[0], uly=roi[1], lrx=roi[2],
                                  lry=roi[3])
        else:
            obs = k.SyntheticBHRObservations(mask, n_train=args.n_train or 500, **syn)
        params, factory = k.TIP_PARAMETERS, k.create_nonlinear_observation_operator
        prior = k.JRCPrior(params, mask)
        prop = k.propagate_information_filter_LAI
        q = np.array([0, 0, 0, 0, 0, 0, 0.04])
        step = 16
    elif args.sensor in ("s2", "multisensor"):
        if args.s2_folder:
            from .input_output.sentinel import Sentinel2Observations
            if not args.emulator_folder:
                raise SystemExit("--s2-folder needs --emulator-folder")
            # a --mask GeoTIFF is the state grid every band is warped onto
            # (kafka_test_S2.py:155-162); without one the granule grid (ROI-cropped)
            obs = Sentinel2Observations(args.s2_folder, args.emulator_folder, args.mask or mask,
                                        roi=None if args.mask else args.roi, decoder=args.in_decoder)
        elif args.sensor == "s2":
            obs = k.SyntheticS2Observations(mask, n_bands=10, n_train=args.n_train or 250, **syn)
        else:
            obs = k.MultiSensorObservations([
                k.SyntheticS2Observations(mask, n_bands=13, n_train=args.n_train or 250, **syn),
                k.SyntheticOLCIObservations(mask, n_bands=21, n_train=args.n_train or 250,
                                            **{**syn, "seed": args.seed + 21})])
        params, factory = k.SAIL_PARAMETERS, k.create_prosail_observation_operator
        prior = k.SAILPrior(params, mask)
        prop, q, step = None, None, 2
    elif args.sensor == "s1":
        if args.s1_folder:       # sigma0_VV / sigma0_VH / theta GeoTIFFs per acquisition
            from .input_output.sentinel import S1Observations
            obs = S1Observations(args.s1_folder, args.mask or mask, roi=None if args.mask else args.roi)
        else:
            obs = k.SyntheticS1Observations(mask, **syn)
        params, factory = ["lai", "sm"], k.create_sar_observation_operator
        prior = k.GaussianPrior(params, mask, [2.0, 0.25], np.diag([1.0, 0.01]))
        prop, q, step = None, None, 6
    elif args.sensor == "identity":
        obs = k.SyntheticIdentityObservations(mask, **syn)
        params, factory = k.TIP_PARAMETERS, k.create_linear_observation_operator
        prior = k.JRCPrior(params, mask)
        prop = k.propagate_information_filter_LAI
        q = np.array([0, 0, 0, 0, 0, 0, 0.04])
        step = 5
    else:
        raise SystemExit(f"unknown sensor {args.sensor}")
    if args.s2_folder or args.s1_folder or args.bhr_folder:   # file readers define the output grid (as the reference drivers)
        projection, geotransform = obs.define_output()
    else:
        projection, geotransform = info.get("projection", ""), info.get("geotransform", [0, 1, 0, 0, 0, -1])

    def make_out(folder):
        """The run's output class and options, writing into ``folder`` (None: device-resident)."""
        physical = getattr(args, "out_physical", None)
        interval = getattr(args, "out_interval", None)
        qa = bool(getattr(args, "out_qa", False))
        if interval is not None and not physical:
            raise SystemExit("--out-interval belongs to --out-physical")
        interval = 0.95 if interval is None else interval
        if not 0.0 < interval < 1.0:
            raise SystemExit("--out-interval LEVEL: a credible level in (0, 1)")
        from .models.transforms import TRANSFORM_TABLES, product_name
        products = [product_name(p, t) for p, t in (TRANSFORM_TABLES[physical].items() if physical else ())
                    if p in params]
        if physical and not products:
            raise SystemExit(f"--out-physical {physical}: none of its parameters is in this run's state "
                             f"({', '.join(params)})")
        if not folder:
            return k.DeviceOutput(params, uncertainty=args.out_unc, physical=physical, level=interval, qa=qa)

        def _ranges(items, flag):
            rg = {}
            for name, lo, hi in items or []:
                if name not in params and not (flag == "--out-range" and name in products):
                    raise SystemExit(f"{flag} {name}: not a parameter of this run ({', '.join(params)})")
                try:
                    rg[name] = (float(lo), float(hi))
                except ValueError:
                    raise SystemExit(f"{flag} {name}: LO and HI are numbers")
            return rg

        scaled = {}
        if args.out_sample == "uint16":
            scaled = dict(sample_type="uint16", ranges=_ranges(args.out_range, "--out-range"),
                          unc_ranges=_ranges(args.out_unc_range, "--out-unc-range"))
        elif args.out_range or args.out_unc_range:
            raise SystemExit("--out-range / --out-unc-range belong to --out-sample uint16")
        return k.KafkaOutput(params, geotransform, projection,
                             folder, prefix=args.prefix, level=args.out_level, gather=args.out_gather,
                             predictor=3 if args.out_fast else 1, strategy="rle" if args.out_fast else None,
                             keep_timesteps=args.out_keep, encoder=args.out_encoder,
                             huffman=args.out_huffman, uncertainty=args.out_unc, physical=physical,
                             interval=interval, qa=qa, **scaled)

    out = make_out(args.out)
    kf = k.LinearKalman(obs, out, mask, factory, params, state_propagation=prop,
                        prior=None if prop is not None else prior, config=cfg, comm=comm, partition=part)
    kf.set_trajectory_model()
    q_scale = float(getattr(args, "q_scale", 1.0) if q_scale is None else q_scale)
    if not (q_scale > 0.0 and np.isfinite(q_scale)):
        raise SystemExit("--q-scale / --scan-q: a scale is a finite number > 0")
    if q is not None:
        kf.set_trajectory_uncertainty(q * q_scale)
    elif q_scale != 1.0:
        raise SystemExit(f"--q-scale / --scan-q: sensor {args.sensor} runs without a model error Q (its state is "
                         "reset to the prior on every step)")
    dates = sorted(obs.dates)
    n = min(args.steps, len(dates)) if args.steps else len(dates)
    grid = [dates[0] - dt.timedelta(days=1)] + [dates[0] + dt.timedelta(days=step * (i + 1) - 1) for i in range(n)]
    return kf, prior, grid, out, make_out, (geotransform, projection)


def _scan_q(args, comm):
    """``--scan-q``: the configured run once per scale of Q, no file output; one
    record per scale and the scale with the largest total log evidence.  Every
    scale is a full filter run: the analysis covariance that feeds the next
    forecast depends on Q, so one trajectory cannot be re-scored under another."""
    recs = []
    for scale in args.scan_q:
        kf, prior, grid, _, _, _ = _build(args, comm, q_scale=scale)
        kf.run(grid, kf.state_from_prior(prior), None, None)
        ev = kf.evidence_summary()
        recs.append({"q_scale": scale, "loglik": ev["loglik"], "d2_per_dof": ev["d2_per_dof"], "dof": ev["dof"]})
        if comm.rank == 0:
            print(json.dumps(recs[-1]), flush=True)
    best = max(recs, key=lambda r: r["loglik"])
    if comm.rank == 0:
        print(json.dumps({"best_q_scale": best["q_scale"], "loglik": best["loglik"]}))
    return recs, best


def cmd_run(args):
    from .parallel import Comm

    import kafka_inferenceengine_amd as k

    if args.scan_q:
        for flag, v in (("--out", args.out), ("--smooth-out", args.smooth_out), ("--resume", args.resume),
                        ("--evidence-out", args.evidence_out)):
            if v:
                raise SystemExit(f"--scan-q repeats the run with file output off: it does not go with {flag}")
    cfg = _engine_config(args)
    comm = Comm.from_env(device=args.device, band_parallel=getattr(args, "band_parallel", None) or 1,
                         timeout_s=cfg.comm_timeout_s)
    if not comm.distributed and comm.band is None:
        import torch
        dev = args.device or ("cuda" if torch.cuda.is_available() else "cpu")
        comm = Comm.single(dev if dev != "cuda" else torch.device("cuda", torch.cuda.current_device()))
    if args.scan_q:
        _scan_q(args, comm)
        comm.destroy()
        return
    kf, prior, grid, out, make_out, geo = _build(args, comm)
    import time
    t_run = time.perf_counter()
    start = None
    if args.resume:
        from .input_output.checkpoint import CheckpointManager
        path = CheckpointManager.resolve(args.resume)
        state = kf.run(grid, None, None, None, resume_from=path)
    else:
        start = kf.state_from_prior(prior)
        state = kf.run(grid, start, None, None)
    t_flush = time.perf_counter()
    if hasattr(out, "flush"):
        out.flush()
    t_end = time.perf_counter()
    smooth_recs = None
    if args.smooth_out:
        sm_out = make_out(args.smooth_out)
        _, smooth_recs = kf.smooth(output=sm_out)
        if hasattr(sm_out, "flush"):
            sm_out.flush()
        fb = [comm.sum_int(r["fallback_pixels"]) for r in smooth_recs]
        t_smooth = time.perf_counter()
    evidence = kf.evidence_summary() if cfg.innovation_evidence else None      # every rank: a rank-ordered sum
    if args.evidence_out:
        from .input_output.evidence import write_evidence_rasters
        ev_files = write_evidence_rasters(args.evidence_out, kf, *geo)
    if comm.rank == 0:
        rec = {"timesteps": len(kf.history), "pixels": kf.n_total,
               "gn_iterations": [h.get("gn_iterations") for h in kf.history],
               "finite": bool(np.isfinite(state.x[:, :state.N].cpu().numpy()).all()),
               # end to end (ingest, assimilation, output drained) and per timestep
               "wall_s": round(t_end - t_run, 3), "output_drain_s": round(t_end - t_flush, 3),
               "timestep_wall_ms": [round(1e3 * h["wall_s"], 1) for h in kf.history if "wall_s" in h]}
        if kf.timer.enabled:
            rec["phases_ms"] = kf.timer.cumulative()
            ing = getattr(kf.observations, "_ingest", None)
            if ing is not None:
                rec["ingest"] = {"bytes_read": ing.bytes_read, "bytes_h2d": ing.bytes_h2d, "pinned": ing.pinned}
        ing = getattr(kf.observations, "_ingest", None)
        if ing is not None and getattr(ing, "decoder", "host") == "device":   # --in-decoder device: what it took
            rec["ingest"] = {"bytes_read": ing.bytes_read, "bytes_h2d": ing.bytes_h2d, "pinned": ing.pinned,
                             "decoder": "device", **ing.stats()}
        ck = getattr(kf, "checkpointer", None)
        if ck is not None and ck.stats["bytes"]:
            rec["checkpoint"] = {k_: [round(v, 3) for v in vals] for k_, vals in ck.stats.items() if k_ != "bytes"}
            rec["checkpoint"]["GB"] = [round(b / 1e9, 2) for b in ck.stats["bytes"]]
        if getattr(out, "write_s", None):
            # writer telemetry: queue depth, engine waits on the writer, encode time, bytes
            rec["output"] = {"files": len(out.written), "write_ms": [round(1e3 * t, 1) for t in out.write_s],
                             **out.writer_stats()}
        if smooth_recs is not None:
            rec["smooth"] = {"out": args.smooth_out, "wall_s": round(t_smooth - t_end, 3),
                             "timesteps": [r["timestep"] for r in smooth_recs], "fallback_pixels": fb,
                             **{k_: [round(1e3 * r.get(k_, 0.0), 1) for r in smooth_recs]
                                for k_ in ("read_s", "h2d_s", "kernel_s", "output_s")},
                             "files": len(getattr(sm_out, "written", []))}
        if evidence is not None:
            rec["evidence"] = evidence
            if args.evidence_out:
                rec["evidence"] = {**evidence, "files": [os.path.basename(p) for p in ev_files]}
        print(json.dumps(rec))
    comm.destroy()


def cmd_farm(args):
    """Independent engine per chunk, chunks round-robin over ranks."""
    import torch

    import kafka_inferenceengine_amd as k
    from .parallel import Comm
    from .parallel.farm import run_chunks

    comm = Comm.from_env(device=args.device)
    mask, _ = _mask(args)
    H, W = mask.shape

    def fn(chunk):
        x0, y0, w, h, no = chunk
        sub = mask[y0:y0 + h, x0:x0 + w]
        dev = comm.device if comm.distributed else torch.device("cuda" if torch.cuda.is_available() else "cpu")
        obs = k.SyntheticBHRObservations(sub, n_train=args.n_train or 200, device=dev, stream=False,
                                         seed=args.seed + no)
        out = k.KafkaOutput(k.TIP_PARAMETERS, None, "", args.out, prefix=hex(no)) if args.out else None
        kf = k.LinearKalman(obs, out, sub, k.create_nonlinear_observation_operator, k.TIP_PARAMETERS, device=dev)
        kf.set_trajectory_uncertainty(np.array([0, 0, 0, 0, 0, 0, 0.025]))
        grid = [obs.dates[0] - dt.timedelta(days=1)] + [d + dt.timedelta(days=1) for d in obs.dates[:args.steps]]
        st = kf.run(grid, kf.state_from_prior(k.JRCPrior(k.TIP_PARAMETERS, sub)), None, None)
        if out is not None:
            out.flush()
        return int(st.N)

    res = run_chunks(W, H, args.block, fn, comm if comm.distributed else None, skip_empty_mask=mask)
    if res is not None:
        print(json.dumps({"chunks": len(res), "pixels": sum(v or 0 for v in res.values())}))
    comm.destroy()


def cmd_synth_s2(args):
    """Write a synthetic Sentinel-2 archive (tiled-DEFLATE GeoTIFF granules +
    emulators) for file-driven runs: ``run --sensor s2 --s2-folder OUT/data
    --emulator-folder OUT/emus``."""
    import torch

    from .input_output.synthetic import synthesize_s2_archive

    h, w = args.size
    dev = args.device or ("cuda" if torch.cuda.is_available() else "cpu")
    data, emus, dates = synthesize_s2_archive(args.out, np.ones((h, w), bool), args.dates, args.n_train, args.seed,
                                              dev, args.cloud)
    print(json.dumps({"data": data, "emulators": emus, "dates": [d.isoformat() for d in dates]}))


def cmd_chunks(args):
    from .input_output.utils import get_chunks

    for c in get_chunks(args.nx, args.ny, args.block):
        print(*c)


def cmd_info(args):
    import torch

    from .ops import SUPPORTED_NP, ext_path

    print(json.dumps({"torch": torch.__version__, "hip": torch.version.hip, "gpu": torch.cuda.is_available(),
                      "device_name": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None,
                      "extension": ext_path(), "compiled_n_params": list(SUPPORTED_NP)}))


def main(argv=None):
    from .engine.config import EngineConfig

    ap = argparse.ArgumentParser(prog="kafka_inferenceengine_amd")
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run", help="assimilation run")
    r.add_argument("--sensor", default="bhr", choices=["bhr", "s2", "s1", "identity", "multisensor"])
    r.add_argument("--size", type=int, nargs=2, default=[512, 512], metavar=("H", "W"))
    r.add_argument("--mask", default=None, help="state mask GeoTIFF (non-zero = active)")
    r.add_argument("--s2-folder", default=None)
    r.add_argument("--emulator-folder", default=None)
    r.add_argument("--bhr-folder", default=None, help="MCD43 kernel rasters A%%Y%%j_kernels_b{0,1}_k{0,1,2}.tif + _qa")
    r.add_argument("--s1-folder", default=None, help="S1_* acquisition folders with sigma0_VV/VH and theta")
    r.add_argument("--emulator", default=None, help="emulator-set .npz for --bhr-folder (default: synthetic TIP)")
    r.add_argument("--period", type=int, default=16, help="take every period-th BHR date")
    r.add_argument("--roi", type=int, nargs=4, default=None, metavar=("ULX", "ULY", "LRX", "LRY"))
    r.add_argument("--steps", type=int, default=0, help="time steps (0: all dates)")
    r.add_argument("--n-train", type=int, default=None)
    r.add_argument("--cloud", type=float, default=0.2)
    r.add_argument("--seed", type=int, default=0)
    r.add_argument("--out", default=None, help="GeoTIFF output folder (default: device-resident output)")
    r.add_argument("--prefix", default=None)
    r.add_argument("--out-level", type=int, default=6, help="DEFLATE level of the output GeoTIFFs (1: fastest)")
    r.add_argument("--out-fast", action="store_true",
                   help="floating-point predictor + run-length DEFLATE (zlib's Z_RLE: about 3x faster encoding "
                        "than zlib level 6; always zlib, also where libdeflate is present -- writer_stats reports "
                        "the encoder)")
    r.add_argument("--out-encoder", default="auto", choices=["auto", "device", "host"],
                   help="DEFLATE tiles encoded on the GPU (device: predictor 3 + fixed-Huffman run-length streams, "
                        "only compressed tiles cross PCIe) or by the host thread pool; auto: device on a GPU")
    r.add_argument("--out-unc", default="conditional", choices=["conditional", "marginal"],
                   help="the _unc rasters: conditional, 1/sqrt(diag(P^-1)) (what the reference writes: every other "
                        "parameter of the pixel held fixed), or marginal, sqrt(diag(P)) (the posterior std of the "
                        "parameter itself; a separate pass over the stored state on every output date)")
    r.add_argument("--out-physical", default=None, choices=["tip", "sail"],
                   help="also write physical-unit products (tip: LAI from TeLAI; sail: cab, car, cw, cm, lai, ala): "
                        "per product NAME_A%%Y%%j.tif with the credible interval's ends _lo.tif / _hi.tif, from a "
                        "separate pass over the stored state on every output date")
    r.add_argument("--out-interval", type=float, default=None, metavar="LEVEL",
                   help="--out-physical: the central credible level of the interval, in (0, 1) (default 0.95)")
    r.add_argument("--out-qa", action="store_true",
                   help="also write QA_A%%Y%%j.tif, one quality byte per pixel (bit legend in the file's metadata; "
                        "255 outside the state mask)")
    r.add_argument("--in-decoder", default="host", choices=["host", "device"],
                   help="--s2-folder granules: DEFLATE tiles inflated by the host thread pool (host), or shipped "
                        "compressed and inflated on the GPU (device: 256 x 256 tiles, 16-bit samples, predictor 1 / 2; "
                        "other files take the host path, file by file)")
    r.add_argument("--out-huffman", default="fixed", choices=["fixed", "dynamic"],
                   help="block type of the device encoder: fixed Huffman codes, or one Huffman table per tile "
                        "built on the GPU wherever that makes the tile smaller (never larger than fixed)")
    r.add_argument("--out-sample", default="float32", choices=["float32", "uint16"],
                   help="sample type of the output GeoTIFFs: float32, or uint16 = scaled 16-bit integers (predictor 2, "
                        "nodata 65535, scale and offset in GDAL_METADATA); uint16 needs --out-range and "
                        "--out-unc-range for every parameter")
    r.add_argument("--out-range", nargs=3, action="append", default=None, metavar=("PARAM", "LO", "HI"),
                   help="--out-sample uint16: the value range [LO, HI] of PARAM's mean raster (repeat per parameter); "
                        "values outside are clamped and counted (writer_stats: saturated)")
    r.add_argument("--out-unc-range", nargs=3, action="append", default=None, metavar=("PARAM", "LO", "HI"),
                   help="--out-sample uint16: the same for PARAM's uncertainty raster")
    r.add_argument("--out-keep", type=int, default=None,
                   help="keep only the newest N timesteps' output files on local disk")
    r.add_argument("--out-gather", action="store_true", help="gather strips to rank 0 and write one raster")
    r.add_argument("--resume", default=None, help="checkpoint directory (latest) or checkpoint path")
    r.add_argument("--smooth-out", default=None, metavar="DIR",
                   help="after the forward run, smooth backward over the steps (RTS) and write the smoothed rasters, "
                        "under the same file names, into DIR; checkpoints every step (into DIR/checkpoints unless "
                        "--checkpoint-dir is given)")
    r.add_argument("--evidence-out", default=None, metavar="DIR",
                   help="implies --innovation-evidence; at the end of the run write evidence_loglik.tif, "
                        "evidence_d2_per_dof.tif, evidence_dof.tif (and, with a gate, evidence_rejected_dates.tif) "
                        "into DIR: the run's per-pixel Gaussian log evidence (linearised at each date's forecast), "
                        "joint chi-square per degree of freedom and observation count")
    r.add_argument("--q-scale", type=float, default=1.0, metavar="S",
                   help="multiply the sensor's built-in model error Q by S")
    r.add_argument("--scan-q", type=float, nargs="+", default=None, metavar="S",
                   help="repeat the run once per scale S of Q with file output off; print one record per scale "
                        "(q_scale, loglik, d2_per_dof, dof) and the scale with the largest total log evidence")
    r.add_argument("--log-level", default="WARNING")
    EngineConfig.add_arguments(r)
    r.set_defaults(fn=cmd_run)
    f = sub.add_parser("farm", help="chunk farming over ranks (kafka_test_Py36.py)")
    f.add_argument("--size", type=int, nargs=2, default=[512, 512], metavar=("H", "W"))
    f.add_argument("--mask", default=None)
    f.add_argument("--block", type=int, nargs=2, default=[256, 256])
    f.add_argument("--steps", type=int, default=4)
    f.add_argument("--n-train", type=int, default=None)
    f.add_argument("--seed", type=int, default=0)
    f.add_argument("--out", default=None)
    f.add_argument("--device", default=None)
    f.set_defaults(fn=cmd_farm)
    y = sub.add_parser("synth-s2", help="write a synthetic Sentinel-2 GeoTIFF archive")
    y.add_argument("--out", required=True)
    y.add_argument("--size", type=int, nargs=2, default=[512, 512], metavar=("H", "W"))
    y.add_argument("--dates", type=int, default=4)
    y.add_argument("--n-train", type=int, default=250)
    y.add_argument("--seed", type=int, default=0)
    y.add_argument("--cloud", type=float, default=0.2)
    y.add_argument("--device", default=None)
    y.set_defaults(fn=cmd_synth_s2)
    c = sub.add_parser("chunks", help="print get_chunks")
    c.add_argument("nx", type=int)
    c.add_argument("ny", type=int)
    c.add_argument("--block", type=int, nargs=2, default=[256, 256])
    c.set_defaults(fn=cmd_chunks)
    i = sub.add_parser("info")
    i.set_defaults(fn=cmd_info)
    args = ap.parse_args(argv)
    if getattr(args, "log_level", None):
        logging.basicConfig(level=getattr(logging, args.log_level.upper()), stream=sys.stderr)
    args.fn(args)


if __name__ == "__main__":
    main()
