"""Fixed-interval (Rauch-Tung-Striebel) smoother: a backward pass over the
filtered states of a finished run.

The forward filter's rasters of a date hold what the observations up to that
date say; the backward pass adds what the later dates say.  Per pixel, with J
the parameters the propagator carries from one time-grid step to the next,
M = diag(m) restricted to J and q the model error::

    x_p = M x_a                 P_p = M P_a M + diag(q)      (on J)
    G   = P_a[:, J] M P_p^-1
    x_s = x_a + G (x_s'[J] - x_p)
    P_s = P_a + G (P_s'[J, J] - P_p) G^T

from the stored filtered (x_a, P_a) of step t and the smoothed (x_s', P_s') of
step t + 1 (``csrc/kf_core.h pixel_smooth``, float64 oracle
``inference.kf_tools.rts_smooth_blocks``).  The reference has no smoother.

For the standard, exact-information and identity propagators the filter's own
forecast is exactly (x_p, P_p): the result is the classical RTS smoother and
equals the batch posterior of the whole series.  The LAI (partial-prior) and
diagonal-approximation propagators forecast with the reference's diagonal
approximation of the precision; the smoother still applies the recursion above
to the stored filtered moments, i.e. it smooths under the transition model,
not under that approximation.
"""
from __future__ import annotations

import logging
import time

import numpy as np
import torch

from ..inference.kf_tools import PROP_PRIOR, PROP_PRIOR_PARTIAL
from ..ops import kernels as K
from .state import COVARIANCE, KFState

LOG = logging.getLogger(__name__)


class SmootherMixin:
    """``LinearKalman.smooth``: see the module docstring."""

    def _smoother_link(self):
        """(prop_mask, m, q): what links two time-grid steps, read from the
        propagator spec and trajectory settings as ``advance_state`` reads them.
        Raises for the configurations the per-pixel recursion does not model."""
        if self.config.spatial_gamma > 0:
            raise ValueError("smooth() with spatial_gamma > 0: under the spatial (GMRF) prior the posterior is not a "
                             "per-pixel quantity, so the per-pixel backward recursion does not apply")
        prop = self._state_propagator
        if prop is not None and self.prior is not None:
            raise ValueError("smooth() with a prior blended with a propagator: the blend is an extra "
                             "pseudo-observation between the steps that the backward recursion does not model")
        n = self.n_params
        if prop is None:
            # no propagator: identity transition, or (with a prior) a reset at every step
            mask = 0 if self.prior is not None else (1 << n) - 1
        else:
            spec = getattr(prop, "device_spec", None)
            if spec is None:
                raise ValueError(f"smooth() needs a propagator with a device_spec (mode, propagated parameters); "
                                 f"{getattr(prop, '__name__', prop)!r} has none")
            if spec.mode == PROP_PRIOR:
                mask = 0
            elif spec.mode == PROP_PRIOR_PARTIAL:
                mask = 0
                for j in spec.propagated:
                    mask |= 1 << int(j)
            else:
                mask = (1 << n) - 1
        return mask, np.asarray(self._m, dtype=np.float64), np.asarray(self._q, dtype=np.float64)

    def _smoother_source(self, checkpoint_dir, states):
        """[(timestep, loader)] in time order; a loader returns the filtered KFState on the device."""
        from ..input_output.checkpoint import CheckpointManager

        if states is not None:
            if checkpoint_dir is not None:
                raise ValueError("smooth(): give checkpoint_dir or states, not both")
            src = sorted(((t, s) for t, s in states), key=lambda e: e[0])

            def held(s):
                def load():
                    s2 = self._materialize(s)
                    s2.require_full("smooth()")
                    return s2
                return load
            return [(t, held(s)) for t, s in src]
        root = checkpoint_dir if checkpoint_dir is not None else self.config.checkpoint_dir
        if root is None:
            raise ValueError("smooth() needs the run's checkpoints (EngineConfig.checkpoint_dir with "
                             "checkpoint_every=1, checkpoint_keep=0), a checkpoint_dir, or states")
        ck = getattr(self, "checkpointer", None)
        if ck is not None:
            ck.finish()
        found = CheckpointManager.committed(root)
        have = {t for t, _ in found}
        # every step of this engine's run must be there
        ran = [r["timestep"] for r in self.history if r.get("event") == "timestep"]
        for iso in ran:
            if not any(t.isoformat() == iso for t in have):
                raise FileNotFoundError(f"smooth(): no committed checkpoint for time step {iso} under {root}; run with "
                                        "checkpoint_every=1 and checkpoint_keep=0 so every step's state is kept")
        if ran:
            found = [(t, p) for t, p in found if t.isoformat() in set(ran)]
        if not found:
            raise FileNotFoundError(f"smooth(): no committed checkpoint under {root}")
        return [(t, (lambda p=p: CheckpointManager.load(p, self)[0])) for t, p in found]

    def _smooth_dump(self, output, timestep, state: KFState):
        if output is None:
            return
        if hasattr(output, "dump_state"):
            output.dump_state(timestep, state, self)
            return
        x, P = state.to_reference()
        if state.kind == COVARIANCE:
            output.dump_data(timestep, x, P, self._as_kind(state, "precision").to_reference()[1],
                             self.partition.local_mask, self.n_params)
        else:
            output.dump_data(timestep, x, None, P, self.partition.local_mask, self.n_params)

    def smooth(self, checkpoint_dir=None, states=None, output=None):
        """Backward (RTS) pass over the filtered states of a finished run.

        The source is the run's committed checkpoints (``checkpoint_dir``,
        default ``config.checkpoint_dir``; the run needs ``checkpoint_every=1,
        checkpoint_keep=0``) or an explicit list ``states`` of
        ``(timestep, KFState)``.  The steps are walked backward with the running
        smoothed state on the device; each step's smoothed state, a ``KFState``
        of kind covariance, is written to ``output`` (any output class; every
        option of it applies as in a forward run).  Each rank smooths its own
        strip; no collective is involved.

        Returns ``(state, records)``: the earliest step's smoothed state and one
        record per step in time order, ``{"timestep", "fallback_pixels",
        "load_s", "kernel_s", "output_s"}`` (wall times, the device
        synchronised between them; from checkpoints also ``read_s`` and
        ``h2d_s``, the parts of ``load_s``); ``fallback_pixels`` counts this
        rank's pixels that kept their filtered state (an input or result that is
        not finite, a block that is not SPD).  The records are logged through
        ``self.metrics`` as ``event="smooth"``.

        Raises ``ValueError`` for a prior blended with a propagator, for
        ``spatial_gamma > 0`` and for a propagator without a ``device_spec``;
        ``FileNotFoundError`` when a step of the run has no committed checkpoint."""
        mask, m, q = self._smoother_link()
        if output is not None and getattr(output, "uncertainty", "conditional") not in ("conditional", "marginal"):
            raise ValueError("output.uncertainty must be 'conditional' or 'marginal'")
        source = self._smoother_source(checkpoint_dir, states)
        n = self.n_params
        sync = (lambda: torch.cuda.synchronize(self.device)) if self.device.type == "cuda" else (lambda: None)
        if mask == 0:
            LOG.info("smooth(): the propagator carries no parameter between the steps; smoothed = filtered")
        records = []
        nxt = None
        for i in range(len(source) - 1, -1, -1):
            timestep, load = source[i]
            t0 = time.perf_counter()
            filt = load()
            if filt.N != self.N or filt.n_params != n:
                raise ValueError(f"smooth(): the state of {timestep.isoformat()} does not match this engine's strip")
            sync()
            t1 = time.perf_counter()
            n_fb = 0
            if mask == 0:
                cur = filt
            elif nxt is None or self.N == 0:
                cur = self._as_kind(filt, COVARIANCE)
            else:
                ld = filt.x.shape[1]
                if nxt.x.shape[1] != ld:
                    nxt = _with_ld(nxt, ld)
                q_pix = self._q_pix
                if q_pix is not None and q_pix.shape[1] != ld:
                    q_pix = _pad_rows(q_pix, ld)
                cur = KFState.empty(n, self.N, self.device, COVARIANCE, ld=ld)
                status = torch.empty(self.N, dtype=torch.uint8, device=self.device)
                K.smooth(n, filt.x, filt.P, nxt.x, nxt.P, cur.x, cur.P, status, kind=filt.kind, prop_mask=mask,
                         m=m, q=q, q_pix=q_pix, N=self.N)
                n_fb = int(status.count_nonzero().item())
            sync()
            t2 = time.perf_counter()
            self._smooth_dump(output, timestep, cur)
            sync()
            t3 = time.perf_counter()
            rec = {"event": "smooth", "timestep": timestep.isoformat(), "fallback_pixels": n_fb,
                   "load_s": t1 - t0, "kernel_s": t2 - t1, "output_s": t3 - t2}
            if states is None:
                rec.update({k: v for k, v in getattr(self, "last_checkpoint_load", {}).items() if k != "bytes"})
            self.metrics.log(rec)
            records.append(rec)
            nxt = cur
        records.reverse()
        return nxt, records


def _pad_rows(t: torch.Tensor, ld: int) -> torch.Tensor:
    out = torch.zeros((t.shape[0], ld), dtype=t.dtype, device=t.device)
    w = min(ld, t.shape[1])
    out[:, :w] = t[:, :w]
    return out


def _with_ld(st: KFState, ld: int) -> KFState:
    return KFState(_pad_rows(st.x, ld), _pad_rows(st.P, ld), st.kind, st.N)
