"""Output writers (plug-in point L1: ``dump_data`` / device ``dump_state``).

* ``KafkaOutput`` — per parameter and timestep a Float32 GeoTIFF of the mean
  and one of 1/sqrt(diag(P^-1)) (the conditional std; ``uncertainty="marginal"``:
  sqrt(diag(P)), the marginal std), file names
  ``{param}_A%Y%j[_{prefix}].tif`` / ``..._unc.tif`` (``observations.py:338-394``).
  Rasters are produced on the device by the unpack kernel and written by a
  background thread.
* ``KafkaOutputMemory`` — in-memory dict {timestep: {param: values}}
  (``kafka_test.py:135-145``; fixed to accept the engine's 6 arguments).
* ``DeviceOutput`` — keeps the latest mean/unc rasters on the device
  (the benchmark's writer: no host traffic in the timed loop).
"""
from __future__ import annotations

import os
import threading
import time
from queue import Queue

import numpy as np
import torch

from ..models.transforms import QA_FILL, QA_LEGEND, TRANSFORM_TABLES, credible_z, resolve_products
from ..ops import kernels as K
from .tiff import write_tiff


UNCERTAINTY_KINDS = ("conditional", "marginal")


def _check_uncertainty(uncertainty):
    if uncertainty not in UNCERTAINTY_KINDS:
        raise ValueError("uncertainty must be 'conditional' or 'marginal'")
    return uncertainty


class ProductSpec:
    """The physical-unit products and the QA layer of an output (``physical=``,
    ``level=``, ``qa=`` of the output classes): ``items`` [(j, name, transform)]
    in state order, ``z`` the interval's half width in standard deviations."""

    def __init__(self, parameter_list, physical=None, level=0.95, qa=False):
        if isinstance(physical, str):
            if physical not in TRANSFORM_TABLES:
                raise ValueError("physical: a mapping parameter -> ParameterTransform, 'tip' or 'sail'")
            physical = TRANSFORM_TABLES[physical]
        self.items = resolve_products(parameter_list, physical)
        if any(name.upper() == "QA" for _, name, _ in self.items) and qa:
            raise ValueError("product name 'QA' collides with the QA layer")
        self.level = float(level)
        self.z = credible_z(level)
        self.qa = bool(qa)
        self.names = [name for _, name, _ in self.items]

    @property
    def active(self) -> bool:
        return bool(self.items) or self.qa

    @property
    def n_sel(self) -> int:
        return len(self.items)

    def table(self, n):
        """One transform (or None) per parameter of an n-parameter state."""
        t = [None] * n
        for j, _, tr in self.items:
            if j >= n:
                raise ValueError("a product's parameter lies outside the state")
            t[j] = tr
        return t

    def metadata(self, s):
        """GDAL_METADATA items of product s's files."""
        _, _, tr = self.items[s]
        return {"TRANSFORM": tr.describe(), "UNITS": tr.units, "LEVEL": repr(self.level)}

    @staticmethod
    def qa_metadata():
        return {f"QA_BIT_{i}": text.split(": ", 1)[1] for i, text in enumerate(QA_LEGEND)} | {"QA_FILL": str(QA_FILL)}

    def from_blocks(self, x_analysis, P, P_inv, n, status=None):
        """The reference-API path: (med, lower, upper [N, n_sel], qa [N]) in
        float64 by ``inference.kf_tools.product_blocks``, from the covariance
        where it was handed in, else the precision blocks."""
        from ..inference.kf_tools import product_blocks
        from ..utils.blocks import sparse_to_blocks
        m = P if P is not None else P_inv
        blocks = m.blocks() if hasattr(m, "blocks") else sparse_to_blocks(m, n)
        x = np.asarray(x_analysis, dtype=np.float64).reshape(-1, n)
        med, lower, upper, qa, _ = product_blocks(x, blocks, self.table(n), self.z,
                                                  kind="covariance" if P is not None else "precision", status=status)
        return med, lower, upper, qa


def _marginal_from_blocks(P, P_inv, n):
    """sqrt(diag(P)) per pixel block in float64, [N, n]: from the covariance
    where it was handed in, else from the inverse of each n x n precision
    block (NaN over a block that cannot be inverted to positive variances)."""
    if P is not None:
        d = np.asarray(P.diagonal(), dtype=np.float64).reshape(-1, n)
    else:
        from ..utils.blocks import sparse_to_blocks
        blocks = P_inv.blocks() if hasattr(P_inv, "blocks") else sparse_to_blocks(P_inv, n)
        blocks = np.asarray(blocks, dtype=np.float64)
        d = np.full((blocks.shape[0], n), np.nan)
        good = np.nonzero(np.isfinite(blocks).all(axis=(1, 2)))[0]
        try:                                     # SPD everywhere (the usual case): one batched call
            np.linalg.cholesky(blocks[good])
        except np.linalg.LinAlgError:
            keep = []
            for i in good:
                try:
                    np.linalg.cholesky(blocks[i])
                    keep.append(i)
                except np.linalg.LinAlgError:
                    pass
            good = np.asarray(keep, dtype=np.int64)
        if good.size:
            d[good] = np.diagonal(np.linalg.inv(blocks[good]), axis1=1, axis2=2)
        d[~(np.isfinite(d) & (d > 0)).all(axis=1)] = np.nan
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(d) & (d > 0), np.sqrt(np.where(d > 0, d, 1.0)), np.nan)


def _fname(folder, param, timestep, prefix, suffix=""):
    core = f"{param}_{timestep.strftime('A%Y%j')}"
    if prefix is not None:
        core += f"_{prefix}"
    return os.path.join(folder, core + suffix + ".tif")


class _Writer:
    """One background thread draining a bounded job queue.  Telemetry:
    ``depth`` (jobs queued or running, sampled at each submit), ``wait_s``
    (seconds the producer -- the engine's host thread -- blocked on a full
    queue) and ``busy_s`` (seconds the thread spent in jobs)."""

    def __init__(self, maxsize: int = 4):
        self.q = Queue(maxsize=maxsize)
        self.err = None
        self.depth = []
        self.wait_s = 0.0
        self.busy_s = 0.0
        self.t = threading.Thread(target=self._run, daemon=True)
        self.t.start()

    def _run(self):
        while True:
            job = self.q.get()
            if job is None:
                return
            t0 = time.perf_counter()
            try:
                job()
            except Exception as e:  # surfaced on flush()
                self.err = e
            finally:
                self.busy_s += time.perf_counter() - t0
                self.q.task_done()

    def submit(self, job):
        if self.err:
            raise self.err
        self.depth.append(self.q.unfinished_tasks)
        t0 = time.perf_counter()
        self.q.put(job)
        self.wait_s += time.perf_counter() - t0

    def flush(self):
        self.q.join()
        if self.err:
            raise self.err


def _device_rasters(state, engine, mean=True, unc=True):   # host copies (tests / tools)
    """(mean, unc) as [n_p, H_strip, W] float32 CPU arrays (inactive = 0)."""
    part = engine.partition
    n = engine.n_params
    H, W = part.strip_shape
    dev = state.x.device
    prec = engine._as_kind(state, "precision")
    m = torch.zeros((n, H * W), dtype=torch.float32, device=dev) if mean else None
    u = torch.zeros((n, H * W), dtype=torch.float32, device=dev) if unc else None
    idx = torch.from_numpy(part.local_idx).to(dev)
    if state.N:
        K.unpack(n, prec.x, prec.P, m, u, idx=idx, N=state.N)
    return (None if m is None else m.view(n, H, W).cpu().numpy(),
            None if u is None else u.view(n, H, W).cpu().numpy())


class KafkaOutput:
    """GeoTIFF writer (``observations.py:338-394``): per parameter and timestep a
    Float32 raster of the mean and one of 1/sqrt(diag(P^-1)).

    Device path: the final Gauss-Newton iteration writes the mean / unc rasters
    straight into device planes (``device_targets``, fused output); the planes
    go to pinned host memory by an async copy on a side stream, and a writer
    thread encodes tiled DEFLATE GeoTIFFs with the native parallel encoder
    (``csrc/kf_tiff.cpp``, EPSG GeoKeys from ``projection``) while the next
    timesteps run.  ``level`` trades size for speed; ``predictor=3,
    strategy="rle"`` (floating-point predictor, run-length zlib) encodes about
    3x faster than level 6 at a similar ratio.
    With ``gather=True`` and several ranks, strips are gathered to rank 0
    (C3, ``Comm.gather_to_root``) and written as one raster; otherwise every
    rank writes its strip with a per-rank prefix and a shifted geotransform.

    ``encoder``: "device" encodes the DEFLATE tiles on the GPU
    (``ops.kernels.TileEncoder``, csrc/kf_deflate.hip: predictor 3 and one
    zlib stream per 256 x 256 tile) on the side stream, so only
    the compressed tiles cross PCIe and the writer thread only writes files;
    "host" sends the raw planes to the native CPU encoder (``level``,
    ``strategy``, ``predictor``); "auto" (default): device for GPU planes with
    DEFLATE output in 256-pixel tiles.

    ``huffman``: the device encoder's block type.  "fixed" (default): one
    fixed-Huffman block per tile.  "dynamic": one Huffman table per tile, built
    on the device from the tile's token histogram, wherever that makes the
    tile smaller (never larger than "fixed"; the files decode the same).  The
    host encoder has no such mode: "dynamic" with ``encoder="host"`` raises.

    ``sample_type``: "float32" (default) or "uint16".  "uint16" writes every
    raster as scaled 16-bit unsigned integers (predictor 2, nodata 65535 for
    NaN, scale and offset in GDAL_METADATA: ``value = offset + scale *
    sample``, ``tiff.read_tiff_scaled``) and needs ``ranges`` and
    ``unc_ranges``: mappings parameter -> ``(lo, hi)`` for the mean and the
    uncertainty rasters; the writer does not guess them.  The device encoder
    quantises in its row load (csrc/kf_deflate.h: ``dfl_quantise``); with
    ``encoder="host"`` (or CPU planes) the host runner of the same quantiser
    produces the same samples and ``write_tiff`` encodes them.  Values outside
    a range are clamped and counted: ``writer_stats()["saturated"]``.

    ``uncertainty``: what the ``_unc`` rasters hold.  "conditional" (default,
    the reference's): 1/sqrt(diag(P^-1)), the spread of a parameter with every
    other parameter of the pixel held fixed.  "marginal": sqrt(diag(P)), the
    posterior std of the parameter on its own (never smaller), computed per
    pixel from the stored analysis state by ``ops.kernels.marginal``; the
    engine then dumps the state after the analysis instead of fusing the
    rasters into it.  A pixel whose precision is not SPD is NaN.  The files
    keep their names and carry an ``UNCERTAINTY`` item in GDAL_METADATA.

    ``physical`` / ``interval`` / ``qa``: physical-unit products with a
    credible interval, and a QA layer.  ``physical``: a mapping parameter ->
    ``models.transforms.ParameterTransform`` (or ``TIP_TRANSFORMS`` /
    ``SAIL_TRANSFORMS``, or "tip" / "sail").  Each listed parameter of
    ``parameter_list`` gets three more files per timestep,
    ``{name}_A%Y%j.tif`` (the transform of the state), ``..._lo.tif`` and
    ``..._hi.tif`` (the ends of the central credible interval of level
    ``interval``, 0.95 by default -- the other output classes call it
    ``level``, which here is the DEFLATE level), ``name`` the transform's or
    ``<parameter>_phys``; GDAL_METADATA carries ``TRANSFORM``, ``UNITS`` and
    ``LEVEL``.  ``qa=True`` adds ``QA_A%Y%j.tif``: one uint8 per pixel
    (``models.transforms.QA_LEGEND``, in the file's metadata; 255 outside the
    state mask), written as it is by the writer thread.  Both come from one
    ``ops.kernels.product`` pass over the stored state after the standard
    planes (the engine then takes the launches ``uncertainty="marginal"``
    takes) and go through the same host / device encoder path as a second
    channel; the standard rasters are those of the unfused run
    (``fuse_output=False``), which in the information form are the fused run's.  With ``sample_type="uint16"``
    a product's range is the transform's physical range where its bounds are
    finite, else ``ranges[name]``."""

    def __init__(self, parameter_list, geotransform, projection, folder, prefix=None, fmt="GTiff",
                 compress="deflate", asynchronous=True, level: int = 6, tile: int = 256, gather: bool = False,
                 threads: int | None = None, predictor: int = 1, strategy: str | None = None,
                 keep_timesteps: int | None = None, encoder: str = "auto", huffman: str = "fixed",
                 sample_type: str = "float32", ranges=None, unc_ranges=None, uncertainty: str = "conditional",
                 physical=None, interval: float = 0.95, qa: bool = False):
        self.uncertainty = _check_uncertainty(uncertainty)
        self.products = ProductSpec(list(parameter_list), physical, interval, qa)
        self.physical, self.interval, self.qa = physical, self.products.level, self.products.qa
        if encoder not in ("auto", "device", "host"):
            raise ValueError("encoder must be 'auto', 'device' or 'host'")
        if huffman not in ("fixed", "dynamic"):
            raise ValueError("huffman must be 'fixed' or 'dynamic'")
        if huffman == "dynamic" and encoder == "host":
            raise ValueError("huffman='dynamic' is a mode of the device encoder (encoder='device' or 'auto')")
        if sample_type not in ("float32", "uint16"):
            raise ValueError("sample_type must be 'float32' or 'uint16'")
        self.sample_type = sample_type
        self._ranges = None       # uint16: ((lo, hi) per parameter) of the mean and of the unc rasters
        if sample_type == "uint16":
            both = []
            for name, rg in (("ranges", ranges), ("unc_ranges", unc_ranges)):
                missing = [p for p in parameter_list if rg is None or p not in rg]
                if missing:
                    raise ValueError(f"sample_type='uint16' needs {name}[param] = (lo, hi); missing: "
                                     + ", ".join(str(p) for p in missing))
                both.append([(float(rg[p][0]), float(rg[p][1])) for p in parameter_list])
                K.TileEncoder.quantiser(both[-1])       # hi <= lo or non-finite bounds: ValueError
            self._ranges = tuple(both)
            # a product's range: the transform's physical range where its bounds are finite (the clamp
            # guarantees it), else ranges[product name]
            prg = []
            for _, name, tr in self.products.items:
                rg_p = ranges[name] if name in ranges else tr.physical_range()
                if rg_p is None:
                    raise ValueError(f"sample_type='uint16': product {name!r} has an unbounded transform and needs "
                                     f"ranges[{name!r}] = (lo, hi)")
                prg.append((float(rg_p[0]), float(rg_p[1])))
            if prg:
                K.TileEncoder.quantiser(prg)
            self._prod_ranges = prg
        elif ranges is not None or unc_ranges is not None:
            raise ValueError("ranges / unc_ranges belong to sample_type='uint16'")
        self.saturated = 0        # uint16: samples clamped to their range so far
        self.saturated_last = {}  # ... per file (base name) of the last timestep written
        self.encoder = encoder
        self.huffman = huffman
        self._enc = None          # ops.kernels.TileEncoder (device encoder)
        self._copier = None       # device encoder: the thread bringing compressed tiles to pinned memory
        self._eslots = {}         # device encoder, per channel: ring of 2 (packed device buffer, meta pinned,
        self._eturn = {}          # host pinned, done)
        self.geotransform = geotransform
        self.projection = projection
        self.folder = folder
        self.fmt = fmt
        self.parameter_list = list(parameter_list)
        self.prefix = prefix
        self.compress = compress
        self.level = int(level)
        self.tile = int(tile)
        self.gather = bool(gather)
        self.threads = threads
        self.predictor = int(predictor)
        self.strategy = strategy
        # rolling local buffer: keep only the newest ``keep_timesteps`` timesteps'
        # files on disk (a node that ships granules elsewhere; benchmarks)
        self.keep_timesteps = keep_timesteps
        self._by_step = []
        os.makedirs(folder, exist_ok=True)
        self._w = _Writer() if asynchronous else None
        self._dev = None          # DeviceOutput: device planes the analysis kernel writes
        self._host = {}           # per channel: pinned host planes in flight (ring of 2)
        self._turn = {}
        self._stream = None
        self.written = []
        self.write_s = []         # per timestep: encode + write wall seconds (writer thread)
        self.bytes_in = self.bytes_out = 0
        self.prune_s = 0.0        # keep_timesteps: removing the older timesteps' files
        self.slot_wait_s = 0.0    # engine thread blocked on a pinned slot still being written
        self.d2h_s = 0.0          # writer thread waiting for the planes' device->host copy

    def _geo(self, engine=None):
        gt = list(self.geotransform) if self.geotransform is not None else None
        if gt is not None and engine is not None and engine.partition.r0 and not self._gathering(engine):
            gt[3] = gt[3] + engine.partition.r0 * gt[5]
        return gt

    def _gathering(self, engine) -> bool:
        return self.gather and engine is not None and engine.comm.world > 1

    def _prefix(self, engine):
        if engine is not None and engine.comm.world > 1 and not self._gathering(engine):
            return f"{self.prefix}_r{engine.comm.rank}" if self.prefix is not None else f"r{engine.comm.rank}"
        return self.prefix

    def _std_groups(self, mean, unc):
        """The standard rasters as file groups: (planes, suffix, uint16 ranges, per-file metadata)."""
        rg = self._ranges if self._ranges is not None else (None, None)
        n = len(self.parameter_list)
        return [(mean, "", rg[0], [self._metadata("")] * n), (unc, "_unc", rg[1], [self._metadata("_unc")] * n)]

    def _write_all(self, timestep, names_in, groups, gt, prefix, extend=False, qa=None):
        """Encode and write the files of one channel: ``groups`` of host planes
        (``_std_groups`` / ``_product_groups``) over the file names ``names_in``;
        ``qa``: the QA plane [H, W] uint8, written with them.  ``extend``: the
        files belong to the timestep whose standard rasters were written last."""
        t0 = time.perf_counter()
        names = []
        u16 = self.sample_type == "uint16"
        sat_last = {}
        for planes, suffix, rg, metas in groups:
            if u16:
                # the host runner of the device encoder's quantiser: the same samples on both paths
                _, _, scale, offset = K.TileEncoder.quantiser(rg)
                planes, sat = K.quantise_u16(np.ascontiguousarray(planes, dtype=np.float32), rg)
            for ii, param in enumerate(names_in):
                fn = _fname(self.folder, param, timestep, prefix, suffix)
                if u16:
                    write_tiff(fn, planes[ii], gt, self.projection, self.compress, level=self.level, tile=self.tile,
                               threads=self.threads, predictor=2, strategy=self.strategy, nodata=65535,
                               scale=scale[ii], offset=offset[ii], metadata=metas[ii])
                    sat_last[os.path.basename(fn)] = int(sat[ii])
                    self.saturated += int(sat[ii])
                else:
                    write_tiff(fn, planes[ii], gt, self.projection, self.compress, level=self.level, tile=self.tile,
                               threads=self.threads, predictor=self.predictor, strategy=self.strategy,
                               metadata=metas[ii])
                self.written.append(fn)
                names.append(fn)
                self.bytes_in += planes[ii].nbytes
                self.bytes_out += os.path.getsize(fn)
        if qa is not None:
            names.append(self._write_qa(timestep, qa, gt, prefix))
        self._written_step(names, sat_last, t0, extend)

    def _write_qa(self, timestep, qa, gt, prefix):
        fn = _fname(self.folder, "QA", timestep, prefix)
        qa = np.ascontiguousarray(qa, dtype=np.uint8)
        write_tiff(fn, qa, gt, self.projection, "deflate", level=self.level, tile=self.tile or 256,
                   threads=self.threads, nodata=QA_FILL, metadata=ProductSpec.qa_metadata())
        self.written.append(fn)
        self.bytes_in += qa.nbytes
        self.bytes_out += os.path.getsize(fn)
        return fn

    def _written_step(self, names, sat_last, t0, extend):
        """Bookkeeping of one channel's files: the product channel (``extend``)
        adds to the timestep its standard rasters opened."""
        u16 = self.sample_type == "uint16"
        if extend and self.write_s:
            if u16:
                self.saturated_last.update(sat_last)
            self.write_s[-1] += time.perf_counter() - t0
            if self.keep_timesteps is not None and self._by_step:
                self._by_step[-1].extend(names)
            return
        if u16:
            self.saturated_last = sat_last
        self.write_s.append(time.perf_counter() - t0)
        self._prune(names)

    def _metadata(self, suffix):
        """Further GDAL_METADATA items of a file: marginal ``_unc`` rasters say so."""
        return {"UNCERTAINTY": "marginal"} if (suffix == "_unc" and self.uncertainty == "marginal") else None

    def _prune(self, names):
        if self.keep_timesteps is not None:
            t1 = time.perf_counter()
            self._by_step.append(names)
            while len(self._by_step) > self.keep_timesteps:
                for fn in self._by_step.pop(0):
                    if os.path.exists(fn):
                        os.remove(fn)
            self.prune_s += time.perf_counter() - t1

    def writer_stats(self) -> dict:
        """Granule output telemetry (per-timestep and cumulative): encode+write
        seconds per timestep, raster bytes in / file bytes out, the writer
        queue's depth at each submit and the seconds the engine blocked on it
        (a full queue, or a pinned host slot still held by its writer job)."""
        w = self._w
        ws = self.write_s
        out = {"timesteps_written": len(ws), "write_s_last": ws[-1] if ws else None,
               "write_s_mean": sum(ws) / len(ws) if ws else None, "write_s_max": max(ws) if ws else None,
               "raster_bytes": self.bytes_in, "file_bytes": self.bytes_out,
               "ratio": round(self.bytes_in / self.bytes_out, 3) if self.bytes_out else None,
               "slot_wait_s": round(self.slot_wait_s, 6), "d2h_s": round(self.d2h_s, 6),
               "prune_s": round(self.prune_s, 6), "deflate_backend": self.deflate_backend(),
               "sample_type": self.sample_type, "uncertainty": self.uncertainty,
               "saturated": {"total": int(self.saturated), "last": dict(self.saturated_last)}}
        if w is not None:
            out.update({"queue_depth_last": w.depth[-1] if w.depth else 0,
                        "queue_depth_max": max(w.depth) if w.depth else 0,
                        "queue_wait_s": round(w.wait_s, 6), "writer_busy_s": round(w.busy_s, 6)})
        return out

    def deflate_backend(self) -> str | None:
        """Encoder of the DEFLATE tiles: libdeflate (default strategy, when the
        host has it) or zlib (always for the rle / huffman strategies)."""
        if self.compress != "deflate":
            return None
        u16 = ", uint16 samples" if self.sample_type == "uint16" else ""
        if self._eslots:
            return f"device ({self.huffman}-Huffman run-length zlib streams{u16}, kf_deflate.hip)"
        from .tiff import _native
        E = _native()
        if E is None or not self.tile:
            return "zlib (python)" + u16
        fast = hasattr(E, "tiff_fast_deflate") and bool(E.tiff_fast_deflate())
        return ("libdeflate" if fast and self.strategy in (None, "default") else "zlib") + u16

    # ------------------------------------------------------- device path
    def _device_output(self):
        if self._dev is None:
            self._dev = DeviceOutput(self.parameter_list, uncertainty=self.uncertainty, physical=self.physical,
                                     level=self.interval, qa=self.qa)
        return self._dev

    def device_targets(self, engine, dev, alias: bool = True):
        return self._device_output().device_targets(engine, dev, alias)

    def mark_written(self, timestep, state, engine):
        self._dev.mark_written(timestep, state, engine)
        self._ship(timestep, engine)

    def dump_state(self, timestep, state, engine, qa_inputs=None):
        self._device_output().dump_state(timestep, state, engine, qa_inputs=qa_inputs)
        self._ship(timestep, engine)

    def _device_encode(self, cuda: bool) -> bool:
        ok = self.encoder != "host" and cuda and self.compress == "deflate" and self.tile == 256
        if self.huffman == "dynamic" and not ok:
            raise ValueError("huffman='dynamic' needs the device encoder: GPU planes, DEFLATE output, 256-pixel tiles")
        if self.encoder == "host" or not cuda or self.compress != "deflate":
            return False
        if self.encoder == "device" and not ok:
            raise ValueError("the device encoder writes 256-pixel tiles")
        return ok

    def _ship(self, timestep, engine):
        """Device planes -> pinned host (async, side stream) -> writer thread.
        Two channels: the standard rasters (mean, unc over the parameters), then
        -- where asked for -- the products (median, lo, hi over the product
        names) with the QA plane; both take the same path."""
        dv = self._dev
        H, W = engine.partition.strip_shape
        gt, pf = self._geo(engine), self._prefix(engine)
        gathering = self._gathering(engine)
        channels = [("std", self.parameter_list, [dv.mean, dv.unc], None)]
        spec = self.products
        if spec.active and (dv.phys is not None or dv.qa_plane is not None):
            ns = spec.n_sel
            channels.append(("prod", spec.names, [dv.phys[g * ns:(g + 1) * ns] for g in range(3)] if ns else [],
                             dv.qa_plane))
        last = None
        for key, names, planes, qa_d in channels:
            Hc = H
            if gathering:
                sizes = [pl.shape[0] for pl in planes]
                parts = list(planes) + ([qa_d.to(torch.float32)[None]] if qa_d is not None else [])
                rows = [b - a for a, b in engine.partition.bounds]
                full = engine.comm.gather_to_root(torch.cat(parts, 0), [r * W for r in rows])
                if engine.comm.rank != 0:
                    continue
                planes, at = [], 0
                for m in sizes:
                    planes.append(full[at:at + m])
                    at += m
                if qa_d is not None:
                    qa_d = full[at].to(torch.uint8)
                Hc = sum(rows)
            cuda = (planes[0] if planes else qa_d).is_cuda
            groups = self._std_groups(*planes) if key == "std" else (self._product_groups(planes) if planes else [])
            if planes and self._device_encode(cuda):
                last = self._ship_encoded(timestep, key, names, groups, qa_d, Hc, W, gt, pf)
            else:
                last = self._ship_planes(timestep, key, names, groups, qa_d, Hc, W, gt, pf, cuda)
        if last is not None and not gathering:
            # the planes' next writer waits for the last copy / encode of this date (DeviceOutput.release)
            self._dev.release(last)

    def _product_groups(self, phys):
        """The product rasters as file groups: ``phys`` the [3 n_sel, ...] planes or
        their three [n_sel, ...] thirds -- median, ``_lo`` and ``_hi``."""
        spec = self.products
        ns = spec.n_sel
        metas = [spec.metadata(i) for i in range(ns)]
        rg = self._prod_ranges if self._ranges is not None else None
        if not isinstance(phys, (list, tuple)):
            phys = [phys[g * ns:(g + 1) * ns] for g in range(3)]
        return [(pl, suffix, rg, metas) for pl, suffix in zip(phys, ("", "_lo", "_hi"))]

    def _ship_planes(self, timestep, key, names, groups, qa_d, H, W, gt, pf, cuda):
        """Host encoder: the raw planes of one channel to pinned memory on the side
        stream, encoded and written by the writer thread.  Returns the copy's event."""
        first = groups[0][0] if groups else qa_d
        if cuda and self._stream is None:
            self._stream = torch.cuda.Stream(first.device)
        n = groups[0][0].shape[0] if groups else 0
        # ring of two pinned buffer sets; a set is reused once its writer job is done
        hbufs, hqa, done = self._next_slot(key, len(groups), n, H * W, cuda, qa_d is not None)
        done.clear()
        ev = None
        if cuda:
            self._stream.wait_stream(torch.cuda.current_stream(first.device))
            with torch.cuda.stream(self._stream):
                for hb, g in zip(hbufs, groups):
                    hb.copy_(g[0][:, :H * W], non_blocking=True)
                if qa_d is not None:
                    hqa.copy_(qa_d[:H * W], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self._stream)
            # an aliased mean (the state's x) is not recycled by the allocator before the copy
            for g in groups:
                g[0].record_stream(self._stream)
        else:
            for hb, g in zip(hbufs, groups):
                hb.copy_(g[0][:, :H * W])
            if qa_d is not None:
                hqa.copy_(qa_d[:H * W])

        def job(ev=ev, done=done):
            try:
                if ev is not None:
                    t0 = time.perf_counter()
                    ev.synchronize()
                    self.d2h_s += time.perf_counter() - t0
                host = [(hb.numpy().reshape(n, H, W),) + tuple(g[1:]) for hb, g in zip(hbufs, groups)]
                self._write_all(timestep, names, host, gt, pf, extend=key != "std",
                                qa=None if hqa is None else hqa.numpy().reshape(H, W))
            finally:
                done.set()

        if self._w is None:
            job()
        elif key != "std" and self._copier is not None:
            # the standard channel went through the device encoder (copier thread, then writer): the
            # same chain, so this timestep's files are written after its standard rasters
            self._copier.submit(lambda: self._w.submit(job))
        else:
            self._w.submit(job)
        return ev

    def _ship_encoded(self, timestep, key, names, groups, qa_d, H, W, gt, pf):
        """Device encoder: every raster group's tiles encoded and packed into one
        device buffer on the side stream, their sizes / offsets to pinned host
        memory; the writer thread then copies exactly the compressed bytes and
        writes the files (no encode on the host).  The QA plane (a byte per
        pixel) goes to pinned memory as it is.  Returns the event after the encode."""
        from ..ops.kernels import TileEncoder
        planes = [g[0] for g in groups]
        G = len(planes)
        n = planes[0].shape[0]
        dev = planes[0].device
        if self._stream is None:
            self._stream = torch.cuda.Stream(dev)
        if self._enc is None:
            self._enc = TileEncoder(huffman=self.huffman, sample=self.sample_type)
        u16 = self.sample_type == "uint16"
        tx, ty = TileEncoder.tiles(H, W)
        per = tx * ty
        nt = n * per
        bound = self._enc.bound()
        # pinned host bytes for the compressed tiles: allocated with the slot (a
        # multi-GB pinned allocation in the writer thread would stall a timed
        # date), sized for the raw planes plus the fixed-Huffman worst case
        host_bytes = int(G * n * H * W * (2 if u16 else 4) * 1.13) + G * nt * 64 + (1 << 20)
        # meta: sizes and offsets of every group's tiles, then (uint16) the planes' saturation counts
        meta_n = 2 * G * nt + (G * n if u16 else 0)
        packed, meta_h, host_box, done = self._next_enc_slot(key, G * nt * bound, meta_n, dev, host_bytes)
        done.clear()
        hqa = None
        if qa_d is not None:
            if len(host_box) < 2 or host_box[1].numel() != H * W:
                del host_box[1:]
                host_box.append(torch.empty(H * W, dtype=torch.uint8, pin_memory=True))
            hqa = host_box[1]
        self._stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(self._stream):
            meta, sats, base = [], [], None
            for pl, g in zip(planes, groups):
                kw = {} if base is None else {"base": base}
                if u16:
                    _, sz, of, q = self._enc.encode(pl, H, W, packed=packed, ranges=g[2], **kw)
                    sats.append(q)
                else:
                    _, sz, of = self._enc.encode(pl, H, W, packed=packed, **kw)
                meta += [sz, of]
                base = of[-1:] + sz[-1:]
            meta_h.copy_(torch.cat(meta + sats), non_blocking=True)
            if hqa is not None:
                hqa.copy_(qa_d[:H * W], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._stream)
        for pl in planes:
            pl.record_stream(self._stream)
        wstream = self._wstream = getattr(self, "_wstream", None) or torch.cuda.Stream(dev)
        gspec = [tuple(g[1:]) for g in groups]

        # two stages on two threads: the copier brings date t + 1's compressed
        # tiles to pinned memory while the writer writes date t's files (the
        # slot -- device packed buffer and pinned bytes -- is released after the
        # write; the ring of two keeps the stages one date apart)
        def write(host, m, done=done):
            try:
                self._write_encoded(timestep, host, m, names, gspec, n, per, H, W, gt, pf, extend=key != "std",
                                    qa=None if hqa is None else hqa.numpy().reshape(H, W))
            finally:
                done.set()

        def copy(packed=packed, meta_h=meta_h, host_box=host_box, ev=ev, done=done):
            try:
                t0 = time.perf_counter()
                ev.synchronize()
                m = meta_h.numpy().copy()
                total = int(m[2 * G * nt - 1] + m[(2 * G - 1) * nt - 1])
                host = host_box[0]
                if host is None or host.numel() < total:
                    host = host_box[0] = torch.empty(int(total * 1.25) + 4096, dtype=torch.uint8, pin_memory=True)
                with torch.cuda.stream(wstream):
                    host[:total].copy_(packed[:total], non_blocking=True)
                wstream.synchronize()
                self.d2h_s += time.perf_counter() - t0
            except BaseException:
                done.set()
                raise
            if self._w is not None:
                self._w.submit(lambda: write(host, m))
            else:
                write(host, m)

        if self._w is not None:
            if self._copier is None:
                self._copier = _Writer()
            self._copier.submit(copy)
        else:
            copy()
        return ev

    def _write_encoded(self, timestep, host, meta, names_in, gspec, n, per, H, W, gt, prefix, extend=False, qa=None):
        from .tiff import write_tiff_tiles
        t0 = time.perf_counter()
        names = []
        nt = n * per
        G = len(gspec)
        so = meta[:2 * G * nt].reshape(2 * G, nt)
        u16 = self.sample_type == "uint16"
        sat_last = {}
        for kind, (suffix, rg, metas) in enumerate(gspec):
            sizes, offs = so[2 * kind], so[2 * kind + 1]
            if u16:
                _, _, scale, offset = K.TileEncoder.quantiser(rg)
                sat = meta[2 * G * nt + kind * n:2 * G * nt + (kind + 1) * n]
            for ii, param in enumerate(names_in):
                fn = _fname(self.folder, param, timestep, prefix, suffix)
                sl = slice(ii * per, (ii + 1) * per)
                if u16:
                    write_tiff_tiles(fn, H, W, host, offs[sl], sizes[sl], gt, self.projection, threads=self.threads,
                                     dtype="uint16", scale=scale[ii], offset=offset[ii], metadata=metas[ii])
                    sat_last[os.path.basename(fn)] = int(sat[ii])
                    self.saturated += int(sat[ii])
                else:
                    write_tiff_tiles(fn, H, W, host, offs[sl], sizes[sl], gt, self.projection, predictor=3,
                                     threads=self.threads, metadata=metas[ii])
                self.written.append(fn)
                names.append(fn)
                self.bytes_in += H * W * (2 if u16 else 4)
                self.bytes_out += os.path.getsize(fn)
        if qa is not None:
            names.append(self._write_qa(timestep, qa, gt, prefix))
        self._written_step(names, sat_last, t0, extend)

    def _next_enc_slot(self, key, packed_bytes, meta_n, dev, host_bytes):
        ring = self._eslots.get(key)
        if not ring or ring[0][0].numel() < packed_bytes or ring[0][1].numel() != meta_n:
            for sl in ring or []:
                sl[3].wait()                # a writer job still reading a slot being replaced
            ring = self._eslots[key] = []
            for _ in range(2):
                ev = threading.Event()
                ev.set()
                ring.append((torch.empty(packed_bytes, dtype=torch.uint8, device=dev),
                             torch.empty(meta_n, dtype=torch.int64, pin_memory=True),
                             [torch.empty(host_bytes, dtype=torch.uint8, pin_memory=True)], ev))
            self._eturn[key] = 0
        slot = ring[self._eturn[key] % 2]
        self._eturn[key] += 1
        t0 = time.perf_counter()
        slot[3].wait()                      # its previous writer job has copied its tiles out
        self.slot_wait_s += time.perf_counter() - t0
        return slot

    def _next_slot(self, key, G, n, cols, cuda, qa):
        sig = (G, n, cols, bool(qa))
        ring = self._host.get(key)
        if not ring or ring[0] != sig:
            pin = cuda and torch.cuda.is_available()
            slots = []
            for _ in range(2):
                ev = threading.Event()
                ev.set()
                slots.append(([torch.empty((n, cols), dtype=torch.float32, pin_memory=pin) for _ in range(G)],
                              torch.empty(cols, dtype=torch.uint8, pin_memory=pin) if qa else None, ev))
            ring = self._host[key] = (sig, slots)
            self._turn[key] = 0
        slot = ring[1][self._turn[key] % 2]
        self._turn[key] += 1
        t0 = time.perf_counter()
        slot[2].wait()                      # its previous writer job has finished with it
        self.slot_wait_s += time.perf_counter() - t0
        return slot

    def dump_data(self, timestep, x_analysis, P_analysis, P_analysis_inv, state_mask, n_params):
        """Reference signature: interleaved x and block-diagonal P^-1."""
        sm = np.asarray(state_mask).astype(bool)
        mean = np.zeros((n_params,) + sm.shape, dtype=np.float32)
        unc = np.zeros_like(mean)
        if self.uncertainty == "marginal":
            sd = _marginal_from_blocks(P_analysis, P_analysis_inv, n_params)
        else:
            d = P_analysis_inv.diagonal()
        for ii in range(n_params):
            mean[ii][sm] = x_analysis[ii::n_params]
            unc[ii][sm] = sd[:, ii] if self.uncertainty == "marginal" else 1. / np.sqrt(d[ii::n_params])
        self._write_all(timestep, self.parameter_list, self._std_groups(mean, unc), self.geotransform, self.prefix)
        if self.products.active:
            # the same definitions in float64 (inference.kf_tools.product_blocks); no status on this path
            spec = self.products
            med, lower, upper, qa = spec.from_blocks(x_analysis, P_analysis, P_analysis_inv, n_params)
            phys = np.zeros((3 * spec.n_sel,) + sm.shape, dtype=np.float32)
            for g, vals in enumerate((med, lower, upper)):
                for i in range(spec.n_sel):
                    phys[g * spec.n_sel + i][sm] = vals[:, i]
            qa_plane = None
            if spec.qa:
                qa_plane = np.full(sm.shape, QA_FILL, dtype=np.uint8)
                qa_plane[sm] = qa
            self._write_all(timestep, spec.names, self._product_groups(phys) if spec.n_sel else [],
                            self.geotransform, self.prefix, extend=True, qa=qa_plane)

    def flush(self):
        if self._copier is not None:
            self._copier.flush()       # its jobs hand their writes to the writer thread
        if self._w is not None:
            self._w.flush()


class KafkaOutputMemory:
    """In-memory output (kafka_test.py:135-145)."""

    def __init__(self, parameter_list, uncertainty: str = "conditional", physical=None, level: float = 0.95,
                 qa: bool = False):
        self.parameter_list = list(parameter_list)
        self.uncertainty = _check_uncertainty(uncertainty)
        self.products = ProductSpec(self.parameter_list, physical, level, qa)
        self.physical, self.level, self.qa = physical, self.products.level, self.products.qa
        self.output = {}

    def dump_data(self, timestep, x_analysis, P_analysis, P_analysis_inv, state_mask, n_params=None):
        n = n_params or len(self.parameter_list)
        sol = {p: np.asarray(x_analysis)[ii::n].copy() for ii, p in enumerate(self.parameter_list)}
        if self.uncertainty == "marginal":
            if P_analysis is not None or P_analysis_inv is not None:
                sd = _marginal_from_blocks(P_analysis, P_analysis_inv, n)
                for ii, p in enumerate(self.parameter_list):
                    sol[p + "_unc"] = sd[:, ii].copy()
        elif P_analysis_inv is not None:
            d = P_analysis_inv.diagonal()
            for ii, p in enumerate(self.parameter_list):
                sol[p + "_unc"] = 1. / np.sqrt(d[ii::n])
        if self.products.active and (P_analysis is not None or P_analysis_inv is not None):
            # physical-unit products: ``name``, ``name_lo``, ``name_hi`` and the ``QA`` bytes
            med, lower, upper, qa = self.products.from_blocks(x_analysis, P_analysis, P_analysis_inv, n)
            for i, name in enumerate(self.products.names):
                sol[name], sol[name + "_lo"], sol[name + "_hi"] = med[:, i].copy(), lower[:, i].copy(), upper[:, i].copy()
            if self.products.qa:
                sol["QA"] = qa
        self.output[timestep] = sol


class DeviceOutput:
    """Keeps the latest analysis rasters on the device (mean and unc planes on
    the strip grid) — the analysis kernel writes them in its final iteration
    (fused output), nothing leaves the GPU unless ``to_host`` is called.

    On a dense strip (every pixel active: the identity raster map) the mean
    raster IS the analysis state's x ([n_p, N] with N = H W), so it is not
    written twice: ``mean`` then references the state's x (``alias_state``;
    a state's buffers are never rewritten -- each date allocates new ones).
    The planes the output owns (the uncertainty planes, and the mean planes of
    a masked strip, the gain form or ``dump_state``) alternate between two
    buffer pairs, so a reader of one date's planes (``KafkaOutput``'s
    device-to-host copy) runs under the next date's analysis;
    ``device_targets`` makes the analysis wait only for a reader of the pair it
    is about to overwrite (``release``).

    ``uncertainty="marginal"``: the uncertainty planes hold sqrt(diag(P))
    instead of 1/sqrt(diag(P^-1)) (see ``KafkaOutput``).  No analysis kernel
    writes that, so the engine does not ask for ``device_targets``: every date
    goes through ``dump_state``, one ``ops.kernels.marginal`` pass over the
    stored state (precision or, for the gain form, covariance) that writes the
    mean planes as well.

    ``physical`` / ``level`` / ``qa``: physical-unit products with a credible
    interval and the QA byte (see ``KafkaOutput``).  They too go through
    ``dump_state``: after the standard planes, one ``ops.kernels.product`` pass
    writes ``phys`` ([3 n_sel, plane]: the medians of the selected parameters,
    then the lower, then the upper ends) and ``qa_plane`` (uint8, 255 outside
    the state mask); ``keep_history`` keeps them in ``product_history``."""

    def __init__(self, parameter_list, keep_history: bool = False, alias_state: bool = True,
                 uncertainty: str = "conditional", physical=None, level: float = 0.95, qa: bool = False):
        self.parameter_list = list(parameter_list)
        self.uncertainty = _check_uncertainty(uncertainty)
        self.products = ProductSpec(self.parameter_list, physical, level, qa)
        self.physical, self.level, self.qa = physical, self.products.level, self.products.qa
        self.phys = None               # [3 n_sel, plane]: median, lower and upper planes of the products
        self.qa_plane = None           # uint8 [plane], QA_FILL outside the state mask
        self.product_history = {}      # keep_history: timestep -> (phys, qa_plane) clones (None where not asked for)
        self._phys_bufs = self._qa_bufs = None
        self.keep_history = keep_history
        self.alias_state = bool(alias_state)
        self.mean = None
        self.unc = None
        self.timestep = None
        self.history = {}
        self._mean_bufs = [None, None]
        self._unc_bufs = None
        self._readers = [None, None]   # event of the last reader of each (mean, unc) buffer pair
        self._turn = 0
        self._alias = False

    def _ensure(self, engine, dev):
        part = engine.partition
        n = engine.n_params
        H, W = part.strip_shape
        if self._unc_bufs is None or self._unc_bufs[0].device != dev or self._unc_bufs[0].shape != (n, H * W):
            self._unc_bufs = [torch.zeros((n, H * W), dtype=torch.float32, device=dev) for _ in range(2)]
            self._mean_bufs = [None, None]
            self._readers = [None, None]
            idx = np.asarray(part.local_idx, dtype=np.int64)
            if idx.size and (idx.min() < 0 or idx.max() >= H * W):
                raise ValueError("partition raster index outside the strip")
            self._idx = torch.from_numpy(idx).to(dev)
            self._identity = part.N == H * W
            self._plane = H * W
            # the product planes alternate with the uncertainty planes (the same reader event guards a pair)
            ns = self.products.n_sel
            self._phys_bufs = [torch.zeros((3 * ns, H * W), dtype=torch.float32, device=dev) for _ in range(2)] \
                if ns else None
            self._qa_bufs = [torch.full((H * W,), QA_FILL, dtype=torch.uint8, device=dev) for _ in range(2)] \
                if self.products.qa else None
        if self.unc is None:
            self.unc = self._unc_bufs[0]

    def _own_mean(self):
        """The mean planes of the current buffer pair (``_turn``): guarded by
        the same reader event as its uncertainty planes."""
        b = self._mean_bufs[self._turn]
        if b is None:
            b = self._mean_bufs[self._turn] = torch.zeros_like(self._unc_bufs[0])
        return b

    def _next_unc(self, dev):
        """The uncertainty buffer of the next date (the other pair than the
        latest), after the last reader of that pair."""
        self._turn ^= 1
        ev = self._readers[self._turn]
        if ev is not None and dev.type == "cuda":
            torch.cuda.current_stream(dev).wait_event(ev)
            self._readers[self._turn] = None
        return self._unc_bufs[self._turn]

    def release(self, event):
        """A reader of the latest planes (recorded after its copy): the
        buffer is not overwritten before it (next-but-one date)."""
        self._readers[self._turn] = event

    def device_targets(self, engine, dev, alias: bool = True):
        """(mean, unc, idx) rasters the analysis kernel can write directly
        (fused output, AnalysisArgs.out_*); followed by ``mark_written``.
        mean None: the state's x is the mean raster (dense strips; ``alias``:
        the caller's kernel writes the final x as the state, the plain
        information-form analysis)."""
        self._ensure(engine, dev)
        unc = self._next_unc(dev)
        self._alias = self.alias_state and self._identity and alias
        self._pending = unc
        return (None if self._alias else self._own_mean()), unc, None if self._identity else self._idx

    def mark_written(self, timestep, state, engine):
        self.timestep = timestep
        self.unc = getattr(self, "_pending", self.unc)
        if self._alias:
            self.mean = state.x[:, :self._plane]
        else:
            self.mean = self._own_mean()
        if self.keep_history:
            self.history[timestep] = (self.mean.clone(), self.unc.clone())

    def dump_state(self, timestep, state, engine, qa_inputs=None):
        """``qa_inputs``: the timestep's (status, nobs, nrej), each uint8 [>= N] on
        the state's device or None -- the inputs of the QA bits 0-3."""
        n = engine.n_params
        self._ensure(engine, state.x.device)
        marginal = self.uncertainty == "marginal"
        # marginal: the state as it is (a covariance state holds the variances on its diagonal rows)
        st = engine._materialize(state) if marginal else engine._as_kind(state, "precision")
        unc = self._next_unc(state.x.device)
        mean = self._own_mean()
        idx = None if self._identity else self._idx
        if state.N and marginal:
            K.marginal(n, st.x, st.P, mean, unc, idx=idx, N=state.N, kind=st.kind)
        elif state.N:
            K.unpack(n, st.x, st.P, mean, unc, idx=idx, N=state.N)
        self._pending, self._alias = unc, False
        if self.products.active:
            # one more pass over the state as it is stored (a covariance state holds the variances
            # on its diagonal rows); the planes of the buffer pair _next_unc has just made current
            spec = self.products
            self.phys = self._phys_bufs[self._turn] if spec.n_sel else None
            self.qa_plane = self._qa_bufs[self._turn] if spec.qa else None
            if state.N:
                sp = st if marginal else engine._materialize(state)
                status, nobs, nrej = qa_inputs if qa_inputs is not None else (None, None, None)
                K.product(n, sp.x, sp.P, spec.table(n), spec.z, phys=self.phys, qa=self.qa_plane, idx=idx,
                          N=state.N, kind=sp.kind, status=status, nobs=nobs, nrej=nrej)
            if self.keep_history:
                self.product_history[timestep] = (None if self.phys is None else self.phys.clone(),
                                                  None if self.qa_plane is None else self.qa_plane.clone())
        self.mark_written(timestep, state, engine)

    def to_host(self, shape=None):
        n = self.mean.shape[0]
        m = self.mean.cpu().numpy()
        u = self.unc.cpu().numpy()
        if shape is not None:
            m, u = m.reshape((n,) + tuple(shape)), u.reshape((n,) + tuple(shape))
        return m, u
