"""End-of-run rasters of the evidence accumulators (``LinearKalman.evidence``,
config.innovation_evidence): four small Float32 GeoTIFFs written once per run
through the host TIFF writer, gathered to rank 0 on a striped run."""
from __future__ import annotations

import os

import numpy as np
import torch

from .tiff import write_tiff

EVIDENCE_FILES = ("evidence_loglik.tif", "evidence_d2_per_dof.tif", "evidence_dof.tif")
REJECTED_FILE = "evidence_rejected_dates.tif"


def evidence_planes(engine) -> dict:
    """file name -> float32 [N] device plane over the engine's active pixels:
    the run's log evidence, joint chi-square per degree of freedom (NaN where
    dof = 0), degrees of freedom and, for a gated run, the dates with a
    rejection (``gate_history``)."""
    ev = engine.evidence
    N, dev = engine.N, engine.device
    if ev is None:      # no date was assimilated
        zero = torch.zeros(N, dtype=torch.float64, device=dev)
        ev = {"loglik": zero, "d2": zero, "dof": torch.zeros(N, dtype=torch.int32, device=dev)}
    dof = ev["dof"].to(torch.float64)
    nan = torch.full_like(dof, float("nan"))
    planes = {EVIDENCE_FILES[0]: ev["loglik"],
              EVIDENCE_FILES[1]: torch.where(dof > 0, ev["d2"] / dof.clamp(min=1), nan),
              EVIDENCE_FILES[2]: dof}
    if engine.config.innovation_gate > 0:
        gh = engine.gate_history
        planes[REJECTED_FILE] = torch.zeros_like(dof) if gh is None else gh.to(torch.float64)
    return {name: p.to(torch.float32) for name, p in planes.items()}


def write_evidence_rasters(folder, engine, geotransform=None, projection=None) -> list[str]:
    """Write the planes of :func:`evidence_planes` on the output grid, NaN on
    inactive pixels, into ``folder``.  Every rank calls this; rank 0 writes and
    returns the paths (the other ranks return [])."""
    part, comm = engine.partition, engine.comm
    planes = evidence_planes(engine)
    H, W = part.strip_shape
    strip = torch.full((len(planes), H * W), float("nan"), dtype=torch.float32, device=engine.device)
    idx = torch.from_numpy(np.flatnonzero(np.asarray(part.local_mask).ravel())).to(engine.device)
    strip[:, idx] = torch.stack(list(planes.values()))
    rows = [b - a for a, b in part.bounds]
    full = comm.gather_to_root(strip, [r * W for r in rows])
    if comm.rank != 0:
        return []
    os.makedirs(folder, exist_ok=True)
    rasters = full.cpu().numpy().reshape(len(planes), sum(rows), W)
    paths = []
    for name, r in zip(planes, rasters):
        path = os.path.join(folder, name)
        write_tiff(path, np.ascontiguousarray(r), geotransform=geotransform, projection=projection or None)
        paths.append(path)
    return paths
