"""Gauss-Newton iteration strategies of ``LinearKalman`` (reference:
``kafka/linear_kf.py:245-307``, the ``while not_converged`` loop of
``do_all_bands``).

``do_all_bands_state`` sets one date's problem up (:class:`_GNRun`) and hands
it to a strategy:

* :meth:`GaussNewtonMixin._gn_global` -- the reference's exit test
  ||x_a - x_prev||_2 / len(x_a) < tol over the engine's whole state (every
  rank's pixels, C1 all-gather), iterations that cannot end the loop queued
  without a host wait, GN 1 + 2 fused into one launch, static convergence of
  linear operators;
* :meth:`GaussNewtonMixin._gn_chunked` -- the same test per get_chunks tile
  (EngineConfig.convergence_chunk, engine/chunks.py), the reference drivers'
  one-LinearKalman-per-chunk semantics (kafka_test_Py36.py:147-187).

The loops only say which iteration they queue and, per chunk, which pixels
it visits (:class:`_Visit`); every iteration's device work in either strategy
goes through :meth:`GaussNewtonMixin._launch`, which decides the rest from
the run: the mode (gain form, spatial prior, band-parallel, split GP path or
the plain fused analysis), GN 1 + 2 in one launch, the stored precision and
output rasters, the norm sinks and the forecast operands.
"""
from __future__ import annotations

import logging
from dataclasses import dataclass

import numpy as np
import torch

from ..ops import kernels as K
from .bands import build_table

LOG = logging.getLogger(__name__.rsplit(".", 1)[0] + ".linear_kf.linear_kf")


@dataclass
class _GNRun:
    """One date's Gauss-Newton problem as set up by do_all_bands_state: the
    operators, the forecast operands (``x_f``, ``P_f``, or None, None and the
    fused ``prop``), the state / precision / status buffers and the launch
    options the iteration strategies (_gn_global, _gn_chunked) and the
    per-mode launches share."""
    specs: list
    dbs: list
    table: object
    precomp: bool
    gain: bool
    bp: bool
    split: object
    prop: object
    x_f: object
    P_f: object
    x_prev: object
    x_new: object
    P_out: object
    status: object
    order: object
    out_t: object
    h0_outs: object
    a_rows: int
    pdiag_rows: int
    len_x: float
    n_bands: int
    fuse2: bool
    fuse_sp: bool
    first_plain: bool
    static_conv: bool


@dataclass
class _Visit:
    """What the per-chunk loop varies per launch: the pixels visited
    (``order[:n_visit]``; n_visit None: all; ``n_visit_dev``: the count read on
    the device, n_visit then only a bound) and the per-pixel norm sink
    (``dn_out``; None on a statically converged date)."""
    order: object
    n_visit: object
    n_visit_dev: object
    dn_out: object


def _swap(x_prev, x_new):
    """The iterate ping-pong: the next iteration linearises at x_new and
    writes over x_prev (allocated here after a first iteration at the fused
    forecast, which has no x_prev)."""
    return x_new, (x_prev if x_prev is not None else torch.empty_like(x_new))


class GaussNewtonMixin:
    """The Gauss-Newton loop strategies and their launches (mixed into LinearKalman)."""

    def _norms_needed_now(self) -> bool:
        """Per-date metrics report the norms as they happen.  Rank-uniform on
        purpose (the metrics path is part of the shared config): the answer
        decides whether this rank queues another collective, so a per-process
        setting such as the log level (INFO often on rank 0 only) must not
        enter it -- INFO lines of statically converged dates are logged when
        the deferred norms resolve."""
        return bool(self.metrics.enabled)

    def resolve_pending(self):
        """Every deferred read-back of the dates run so far: the norms of
        statically converged dates and the per-chunk iteration histograms."""
        self._resolve_lazy_norms()
        if self._chunks is not None:
            self._chunks.resolve()

    def _resolve_lazy_norms(self):
        """Fill in the deferred norms of statically converged dates (linear
        operators): iteration 1's norm, and a check that iteration 2's is 0."""
        while self._lazy_norms:
            norms, p1, p2, len_x, nb = self._lazy_norms.pop(0)
            norms[0] = self._log_norm(p1.result(), len_x, nb, 1)
            n2 = p2.result()
            if n2 != 0.0:
                LOG.warning("linear operator: second Gauss-Newton norm %g is not 0", n2)
                norms[1] = self._log_norm(n2, len_x, nb, 2)

    @staticmethod
    def _log_norm(total: float, len_x: float, n_bands: int, n_iter: int) -> float:
        """convergence_norm = ||x_a - x_prev||_2 / len(x_a) (linear_kf.py:293-296)."""
        convergence_norm = float(np.sqrt(max(total, 0.0)) / len_x)
        LOG.info("Band {:d}, Iteration # {:d}, convergence norm: {:g}".format(n_bands - 1, n_iter,
                                                                             convergence_norm))
        return convergence_norm

    def _gn_global(self, run: "_GNRun"):
        """Gauss-Newton loop with the reference's exit test over this engine's
        whole state (linear_kf.py:293-304: ||x_a - x_prev|| / len(x_a) over every
        rank's pixels, C1).  Iterations that cannot end the loop are queued
        without waiting for their norm; GN 1 + 2 run in one launch where the
        first cannot end it (fuse_gn); linear operators converge statically.
        Returns (x, iterations, norms)."""
        cfg = self.config
        N = self.N
        n_iter = 1
        norms, deferred = [], []
        x_prev, x_new = run.x_prev, run.x_new
        while True:
            self._rebuild_table(run, x_prev)
            fused = run.fuse2 or run.fuse_sp
            if fused:
                # iterations 1 + 2 in one launch: outputs of iteration 2 (which can end the loop)
                red2 = self._red_hist[1:3]
                with self.timer.phase("analysis"):
                    if N:
                        self._launch(run, x_prev, x_new, n_iter, True)
                        K.reduce_partials(self._partials1, red2[0:1])
                        K.reduce_partials(self._partials, red2[1:2])
                    else:
                        red2.zero_()
                with self.timer.phase("converge"):
                    pend2 = self.comm.sum_f64_async(red2)
                run.fuse2 = run.fuse_sp = False
                deferred.append((1, pend2.column(0)))
                pend = pend2.column(1)
                n_iter = 2
            else:
                with self.timer.phase("analysis"):
                    if N:
                        self._launch(run, x_prev, x_new, n_iter, False)
                red = self._red_hist[min(n_iter, self._red_hist.numel() - 1):][:1]
                with self.timer.phase("analysis"):
                    if N:
                        K.reduce_partials(self._partials, red)
                    else:
                        red.zero_()
                with self.timer.phase("converge"):
                    pend = self.comm.sum_f64_async(red)
            x_prev, x_new = _swap(x_prev, x_new)
            if fused and run.static_conv and not self._norms_needed_now():
                # norm 2 is exactly 0: converged.  Norm 1 is read after the
                # next launch is queued (no host wait between the steps)
                self._run_lookahead()
                self._resolve_lazy_norms()
                norms = [None, 0.0]
                self._lazy_norms.append((norms, deferred[0][1], pend, run.len_x, run.n_bands))
                return x_prev, n_iter, norms
            if n_iter < cfg.min_iterations:
                # this iteration cannot end the loop (n_iter <= max_iterations too):
                # queue the next one without waiting for the norm
                deferred.append((n_iter, pend))
                n_iter += 1
                continue
            self._run_lookahead()
            self._resolve_lazy_norms()
            for it, pd in deferred:
                norms.append(self._log_norm(pd.result(), run.len_x, run.n_bands, it))
            deferred = []
            convergence_norm = self._log_norm(pend.result(), run.len_x, run.n_bands, n_iter)
            norms.append(convergence_norm)
            if convergence_norm < cfg.convergence_tolerance and n_iter >= cfg.min_iterations:
                return x_prev, n_iter, norms
            if n_iter > cfg.max_iterations:
                LOG.warning("Bailing out after 25 iterations!!!!!!")
                return x_prev, n_iter, norms
            n_iter += 1

    def _run_lookahead(self):
        """The next date's host preparation (LinearKalman._prepare_date), once,
        under the kernels just queued: called after the launch that can end
        the loop and before the first blocking read of a norm or decision."""
        if self._lookahead_fn is not None:
            self._lookahead_fn()
            self._lookahead_fn = None

    def _rebuild_table(self, run: "_GNRun", x_prev):
        """OP_PRECOMP bands (reference-protocol factories): evaluate them on the
        host at this iteration's linearisation point and rebuild the band
        table into ``run.table``, where the launches and the Hessian pass
        after the loop read it."""
        if run.precomp:
            pre = self._precompute_host(run.specs, run.dbs, x_prev)
            run.table = build_table(run.specs, run.dbs, self.n_params, self._cache, self.device, run.h0_outs, pre)

    def _launch(self, run: "_GNRun", x_prev, x_new, n_iter, fused, visit: "_Visit | None" = None):
        """One Gauss-Newton iteration's device work (``fused``: iterations 1
        and 2 in one launch), by mode: the gain form (K1g), the spatial prior's
        plain first iteration or regularised solve (K9 + C2), band-parallel
        (C5), the split GP path, or the plain fused analysis (K1).  ``visit``:
        the per-chunk loop's visiting subset and per-pixel norms; without it
        the launch visits every pixel and writes the tile-wide norm partials."""
        cfg = self.config
        n = self.n_params
        # the analysis precision and the output rasters are only needed from the
        # iteration that can end the loop on: skip the 4*ntri B/px store before
        # min_iterations.  The fused pair always stores (min_iterations > 2 too)
        store = fused or n_iter >= cfg.min_iterations
        P_out, out = (run.P_out, run.out_t) if store else (None, None)
        if visit is None:
            partials, first = self._partials, self._partials1 if fused else None
            kw = dict(order=run.order)
        else:
            partials, first = None, None
            kw = dict(order=visit.order, n_visit=visit.n_visit, n_visit_dev=visit.n_visit_dev, dn_out=visit.dn_out)
        kw.update(N=self.N, prop=run.prop, gn_fused=2 if fused else 1, partials_first=first, line=self._line_opt)
        if run.gain:
            K.gain(n, run.table, x_prev, run.x_f, run.P_f, x_new, P_out, run.status, partials, joseph=cfg.joseph,
                   out=out, pdiag_rows=run.pdiag_rows if store else 0, **kw)
        elif run.first_plain and n_iter == 1 and not fused:
            # the unfused form of fuse_sp's first iteration (same kernel path)
            K.analysis(n, run.table, x_prev, run.x_f, run.P_f, x_new, None, None, run.status, partials, **kw)
            self._reg_log.append({"solver": "plain", "rho": 0.0, "sweeps": 0, "r2": None, "count": 0})
        elif cfg.spatial_gamma > 0:
            self._regularised_iteration(run, x_prev, x_new, P_out, out, final=store, partials_first=first)
        elif run.bp:
            self._band_parallel_iteration(run, x_prev, x_new, P_out, visit)
        elif run.split is not None:
            self._split_iteration(run, x_prev, x_new, P_out)
        else:
            K.analysis(n, run.table, x_prev, run.x_f, run.P_f, x_new, P_out, None, run.status, partials, out=out,
                       a_rows=run.a_rows, **kw)

    def _chunk_state(self):
        from .chunks import ChunkConvergence

        cc = self._chunks
        block = tuple(int(v) for v in self.config.convergence_chunk)
        if cc is None or cc.block != block:
            cc = self._chunks = ChunkConvergence(self.partition, block, self.n_params, self.device, self.comm)
        return cc

    def _gn_chunked(self, run: "_GNRun"):
        """Gauss-Newton loop with the exit test per chunk (engine/chunks.py;
        reference: one LinearKalman per get_chunks tile, kafka_test_Py36.py:147-187,
        each testing ||x_a - x_prev|| / len(x_a) < tol, linear_kf.py:293-304).

        Every launch writes each visited pixel's |dx|^2; after each iteration
        that can end the loop the chunks are tested (one C1 all-gather of the
        per-chunk partials), and the next launch visits only the pixels of the
        chunks still iterating (the stopped chunks' x, precision, outputs and
        status stay as their last iteration wrote them).  Returns (x, the
        largest chunk's iteration count, the largest tested norm per
        iteration)."""
        cfg = self.config
        N = self.N
        cc = self._chunk_state()
        # linear operators: iteration 2 repeats iteration 1 exactly, so every
        # chunk's norm is 0 and every chunk stops at iteration 2 -- the decision
        # is known without the per-chunk norms' read-back (static_conv implies
        # the fused first launch, run.fuse2)
        static = run.static_conv and not self._norms_needed_now()
        if not static and not cc.ready:
            cc.begin()          # (normally queued at the end of the previous date, off this date's host path)
        x_prev, x_new = run.x_prev, run.x_new
        n_iter, n_visit, vis, full = 1, N, run.order, True
        norms = []
        # the tail past the first decision that keeps chunks iterating: up to
        # ``gn_lookahead`` iterations queued ahead of the read-backs, each
        # launch / compaction reading its pixel count on the device (n_dev);
        # n_visit stays a host bound (the last count read: counts only shrink)
        depth = cfg.gn_lookahead if not (run.bp or run.precomp) else 0
        pending = []            # (iteration, its decision) not read yet
        tail, n_dev, n_end = False, None, None
        while True:
            self._rebuild_table(run, x_prev)
            fused = run.fuse2 and n_iter == 1
            with self.timer.phase("analysis"):
                if N and n_visit:
                    self._launch(run, x_prev, x_new, n_iter, fused,
                                 _Visit(vis, None if full else n_visit, n_dev, None if static else cc.dn))
            if n_iter == 1:
                cc.resolve()    # the previous dates' histograms, under this launch (read-backs done long ago)
            if fused:
                n_iter = 2
            x_prev, x_new = _swap(x_prev, x_new)
            if static:
                self.last_chunk_iters = cc.set_static(n_iter)
                return x_prev, n_iter, [0.0]
            if n_iter < cfg.min_iterations:
                n_iter += 1
                continue
            with self.timer.phase("converge"):
                pending.append((n_iter, cc.decide(n_iter, cfg.convergence_tolerance, cfg.min_iterations,
                                                  cfg.max_iterations)))
            self._run_lookahead()
            read = None
            # read the oldest decision unless the tail may queue one more iteration first
            while pending and not (tail and len(pending) <= depth and n_iter <= cfg.max_iterations):
                k, pend = pending.pop(0)
                n_act, mx, px, n_new = (pend.result(j) for j in range(4))
                n_act, px = int(n_act), int(px)
                norms.append(float(mx))
                LOG.info("Iteration # %d: %d of %d chunks converged, %d still iterating, largest chunk norm %g",
                         k, int(n_new), cc.tested, n_act, mx)
                if n_act == 0:
                    n_end = k           # the later queued iterations (if any) visit nothing
                    break
                if k > cfg.max_iterations:      # chunk_decide bails every chunk out past max_iterations
                    raise RuntimeError("per-chunk loop past max_iterations with active chunks")
                read = (k, px)
                tail = depth > 0
            if n_end is not None:
                break
            # queue iteration n_iter + 1: its pixel count is exact when this
            # iteration's decision was just read, else on the device only
            exact = read is not None and read[0] == n_iter
            with self.timer.phase("converge"):
                vis = cc.compact(vis, n_visit if N else 0, read[1] if exact else None, x_prev, x_new, n_in_dev=n_dev)
            if read is not None:
                n_visit = min(n_visit, read[1])
            n_dev = None if exact else cc.px_slot(n_iter)
            full = False
            n_iter += 1
        n_iter = n_end
        def bail(hist, max_it=cfg.max_iterations):
            if max(hist or {0: 0}) > max_it:
                LOG.warning("Bailing out after 25 iterations!!!!!!")
        # per-date metrics serialise the record now; otherwise the histogram is
        # read back without draining the stream (filled in by the next date)
        self.last_chunk_iters = cc.histogram() if self._norms_needed_now() else cc.histogram_async(bail)
        if self._norms_needed_now():
            bail(self.last_chunk_iters)
        cc.begin()              # the next date's reset, queued behind this date's read-backs
        return x_prev, n_iter, norms
