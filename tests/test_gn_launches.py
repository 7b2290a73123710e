"""The engine's launch trace per configuration: which K.analysis / K.gain /
K.reg_finish / K.gp_operator launches three dates queue, in order, with which
operands absent and which options set (engine/gn.py decides them: the stored
precision and output rasters per iteration, pdiag_rows, the norm sinks, the
fused forecast's operands, the per-chunk visiting subset).

The expected traces (tests/golden/gn_launches.json) are recorded by running
this module as a script (``python tests/test_gn_launches.py``) on the host
runner; the file names the commit they were recorded at.  Nothing recorded
depends on the device, so the GPU runs are held to the same traces."""
import datetime as dt
import inspect
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import kafka_inferenceengine_amd as k                      # noqa: E402
from kafka_inferenceengine_amd.ops import kernels as K     # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gn_launches.json")
RECORDED = ("analysis", "gain", "reg_finish", "gp_operator")
TENSORS = ("x_prev", "x_f", "pf_inv", "p_f", "x_out", "a_out", "p_out", "b_out", "status", "partials",
           "partials_first", "order", "n_visit_dev", "dn_out", "a_in", "x0_out", "prop", "reg")
SCALARS = ("gn_fused", "n_visit", "a_rows", "pdiag_rows", "solve", "joseph")


class _Trace:
    """Recorders around the launch functions of ops.kernels (the engine
    modules call them as ``K.…``); each forwards to the real function."""

    def __init__(self, setattr_):
        self.launches = []
        self._last_x_out = None
        for name in RECORDED:
            setattr_(K, name, self._wrap(name, getattr(K, name)))

    def _wrap(self, name, fn):
        sig = inspect.signature(fn)

        def recorder(*args, **kw):
            bound = sig.bind(*args, **kw)
            bound.apply_defaults()
            self._record(name, bound.arguments)
            return fn(*args, **kw)
        return recorder

    def _record(self, name, a):
        none = [t for t in TENSORS if t in a and a[t] is None]
        if "out" in a:
            none += ["out[%d]" % i for i in range(3) if a["out"] is None or a["out"][i] is None]
        e = {"fn": name, "none": " ".join(none)}
        if "x_prev" in a:
            xp, last = a["x_prev"], self._last_x_out
            e["x_prev_is_last_x_out"] = bool(xp is not None and last is not None
                                             and xp.data_ptr() == last.data_ptr() and xp.shape == last.shape)
        if "x_out" in a:
            self._last_x_out = a["x_out"]
        for s in SCALARS:
            if s in a:
                e[s] = a[s] if a[s] is None or isinstance(a[s], bool) else int(a[s])
        self.launches.append(e)


# ----------------------------------------------------------- configurations
def _tip(device, out=False, **cfg):
    """The 24 x 20 JRC-TIP problem of tests/test_engine.py:_setup, three dates."""
    mask = np.ones((24, 20), bool)
    mask[:3, :4] = False
    obs = k.SyntheticBHRObservations(mask, n_train=80, stream=False, n_pool=5, device=device, seed=0, field_cell=8)
    x0, Pinv = k.JRCPrior(k.TIP_PARAMETERS, mask).process_prior(None)
    Q = np.zeros_like(x0)
    Q[6::7] = 0.04
    kf = k.LinearKalman(obs, k.DeviceOutput(k.TIP_PARAMETERS) if out else None, mask,
                        k.create_nonlinear_observation_operator, k.TIP_PARAMETERS,
                        state_propagation=k.propagate_information_filter_LAI, device=device,
                        config=k.EngineConfig(**cfg))
    kf.set_trajectory_model()
    kf.set_trajectory_uncertainty(Q)
    grid = [dt.datetime(2017, 1, 1) + dt.timedelta(days=16 * i) for i in range(4)]
    return lambda: kf.run(grid, x0, None, Pinv)


def _split(device, chunk):
    """tests/test_engine.py:test_split_gp_operator_path_equals_fused, gp_split="always"."""
    mask = np.ones((10, 9), bool)
    obs = k.SyntheticS2Observations(mask, n_bands=10, n_train=30, device=device, stream=False, n_pool=2,
                                    field_cell=4)
    prior = k.SAILPrior(k.SAIL_PARAMETERS, mask)
    x0, Pinv = prior.process_prior(None)
    grid = [obs.dates[0] - dt.timedelta(days=1), obs.dates[2] + dt.timedelta(days=1)]
    kf = k.LinearKalman(obs, None, mask, k.create_prosail_observation_operator, k.SAIL_PARAMETERS,
                        state_propagation=None, prior=prior, device=device,
                        config=k.EngineConfig(gp_split="always", band_chunk=chunk, return_innovations=True))
    return lambda: kf.run(grid, x0, None, Pinv)


def _identity(device, **cfg):
    """tests/test_engine.py:test_linear_operator_converges_statically."""
    mask = np.ones((20, 24), bool)
    dates = [dt.datetime(2017, 1, 1) + dt.timedelta(days=16 * i) for i in range(3)]
    obs = k.SyntheticIdentityObservations(mask, dates=dates, device=device, seed=3, stream=False)
    kf = k.LinearKalman(obs, None, mask, k.create_linear_observation_operator, k.TIP_PARAMETERS,
                        state_propagation=k.propagate_information_filter_LAI, device=device,
                        config=k.EngineConfig(**cfg))
    kf.set_trajectory_uncertainty(np.array([0, 0, 0, 0, 0, 0, 0.04]))
    x0, Pi = k.JRCPrior(k.TIP_PARAMETERS, mask).process_prior(None)
    grid = [dates[0] - dt.timedelta(days=1)] + [d + dt.timedelta(days=1) for d in dates]
    return lambda: kf.run(grid, x0, None, Pi)


_HARD_EMULATORS = {}


def _hard(device, lookahead, form):
    """The hard PROSAIL problem of tests/test_chunks.py:_chunked_run (chunks
    iterate past the first decision: the tail and its device-side counts)."""
    import test_chunks as tc

    kf, obs, prior = tc._engine(tc._mask(), {"convergence_chunk": [tc.BLOCK, tc.BLOCK], "gn_lookahead": lookahead,
                                             "analysis_form": form}, emulators=_HARD_EMULATORS.get(device),
                                device=device)
    _HARD_EMULATORS[device] = obs.emulators
    return lambda: kf.run(tc.GRID, kf.state_from_prior(prior), None, None)


SPATIAL = dict(out=True, spatial_gamma=5.0, spatial_params=[6], max_iterations=4)
CONFIGS = {
    "information": lambda d: _tip(d),
    "information-unfused": lambda d: _tip(d, fuse_gn=False),
    "gain-output": lambda d: _tip(d, out=True, analysis_form="gain"),
    "gain-output-unfused": lambda d: _tip(d, out=True, analysis_form="gain", fuse_gn=False),
    "chunked-information": lambda d: _tip(d, convergence_chunk=[8, 8]),
    "chunked-gain": lambda d: _tip(d, convergence_chunk=[8, 8], analysis_form="gain"),
    "hessian": lambda d: _tip(d, hessian_correction=True),
    "hessian-chunked": lambda d: _tip(d, hessian_correction=True, convergence_chunk=[8, 8]),
    "spatial": lambda d: _tip(d, **SPATIAL),
    "spatial-unfused": lambda d: _tip(d, fuse_gn=False, **SPATIAL),
    "split-10": lambda d: _split(d, 10),
    "split-3": lambda d: _split(d, 3),
    "identity": lambda d: _identity(d),
    "identity-chunked": lambda d: _identity(d, convergence_chunk=[8, 8]),
    "hard-information-lookahead0": lambda d: _hard(d, 0, "information"),
    "hard-information-lookahead2": lambda d: _hard(d, 2, "information"),
    "hard-gain-lookahead0": lambda d: _hard(d, 0, "gain"),
    "hard-gain-lookahead2": lambda d: _hard(d, 2, "gain"),
}


def _trace(name, device, setattr_):
    run = CONFIGS[name](device)
    tr = _Trace(setattr_)
    run()
    return tr.launches


_GOLDEN = None


def _expected(name):
    global _GOLDEN
    if _GOLDEN is None:
        with open(GOLDEN) as f:
            _GOLDEN = json.load(f)
    return [_GOLDEN["launches"][i] for i in _GOLDEN["traces"][name]]


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)])
def test_launch_trace(device, name, monkeypatch, request):
    if device == "cuda":
        device = request.getfixturevalue("cuda")
    got = _trace(name, device, monkeypatch.setattr)
    want = _expected(name)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"launch {i} of {len(got)}"
    assert len(got) == len(want)


if __name__ == "__main__":
    import subprocess

    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True,
                            check=True).stdout.strip()
    launches, traces = [], {}
    for name in CONFIGS:
        with pytest.MonkeyPatch.context() as mp:
            seq = _trace(name, "cpu", mp.setattr)
        traces[name] = []
        for e in seq:
            if e not in launches:
                launches.append(e)
            traces[name].append(launches.index(e))
        print(name, len(seq), "launches")
    with open(GOLDEN, "w") as f:
        f.write("{\n \"commit\": %s,\n \"launches\": [\n  " % json.dumps(commit))
        f.write(",\n  ".join(json.dumps(e) for e in launches))
        f.write("\n ],\n \"traces\": {\n  ")
        f.write(",\n  ".join("%s: %s" % (json.dumps(n), json.dumps(t)) for n, t in traces.items()))
        f.write("\n }\n}\n")
