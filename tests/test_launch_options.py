"""The launch options K.analysis and K.gain share (visiting order, norm
partials, output rasters, SoA operands, the fused-forecast handle): every
refusal holds in both forms, and one launch with all of them set runs.

Host runner, n = 2 states, N = 8 pixels, one linear band."""
import numpy as np
import pytest
import torch

from kafka_inferenceengine_amd.ops import kernels as K

import kernel_cases as C

n, N, NT = 2, 8, 3
FORMS = ("analysis", "gain")


def _launch(form, fused=True, **over):
    """One launch at the fused forecast with every shared option set correctly,
    then ``over`` applied (``p_out``: the packed output of either form)."""
    c = C.nongp_case(n, N, (("linear", K.OBS_F32),), fused=True)
    tab, _ = C.nongp_table(c, "cpu", 0)
    pa = c["pa"] if form == "analysis" else np.linalg.inv(c["pa"])    # K1g: the analysis covariance
    prop = K.prop_args(n, c["spec"], C.soa(c["xa"], "cpu"), C.packed(pa, "cpu"), fused=fused)
    kw = dict(x_out=torch.zeros((n, N)), p_out=torch.zeros((NT, N)), status=torch.zeros(N, dtype=torch.uint8),
              partials=K.partials_buffer(N, "cpu"), N=N, prop=prop,
              order=torch.arange(N - 1, -1, -1, dtype=torch.int32), n_visit=5,
              n_visit_dev=torch.tensor([4], dtype=torch.int32), dn_out=torch.zeros(N), gn_fused=1,
              partials_first=K.partials_buffer(N, "cpu"),
              out=(torch.zeros((n, N + 2)), torch.zeros((n, N + 2)), torch.arange(2, N + 2, dtype=torch.int64)))
    kw.update(over)
    if form == "analysis":
        kw["a_out"] = kw.pop("p_out")
    getattr(K, form)(n, tab, None, None, None, **kw)
    return kw


def _planes(mean, unc, idx=None):
    return (None if mean is None else torch.zeros((n, mean)), torch.zeros((n, unc)), idx)


REFUSALS = {
    "n_visit without order": dict(order=None),
    "n_visit out of range": dict(n_visit=N + 1),
    "n_visit zero": dict(n_visit=0),
    "n_visit with gn_fused=2": dict(gn_fused=2),
    "n_visit_dev without n_visit": dict(n_visit=None),
    "order dtype": dict(order=torch.arange(N, dtype=torch.int64)),
    "dn_out dtype": dict(dn_out=torch.zeros(N, dtype=torch.float64)),
    "gn_fused=3": dict(gn_fused=3, n_visit=None, n_visit_dev=None),
    "partials_first too small": dict(partials_first=torch.zeros(0, dtype=torch.float64)),
    "out planes differ": dict(out=_planes(N, N + 1)),
    "out idx dtype": dict(out=_planes(N, N, torch.arange(N, dtype=torch.int32))),
    "out mean None with idx": dict(out=_planes(None, N, torch.arange(N, dtype=torch.int64))),
    "identity out, plane < N": dict(out=_planes(N - 1, N - 1)),
    "leading dimensions differ": dict(p_out=torch.zeros((NT, N + 1))),
    "prop not fused": dict(fused=False),
}


@pytest.mark.parametrize("what", list(REFUSALS))
@pytest.mark.parametrize("form", FORMS)
def test_shared_option_refused(form, what):
    with pytest.raises(ValueError):
        _launch(form, **REFUSALS[what])


@pytest.mark.parametrize("form", FORMS)
def test_shared_options_accepted(form):
    kw = _launch(form)
    visited = kw["order"][:4].long()       # n_visit_dev = 4 of the n_visit = 5 slots
    mean, unc, idx = kw["out"]
    assert torch.equal(mean[:, idx[visited]], kw["x_out"][:, visited]) and bool((unc[:, idx[visited]] > 0).all())
    rest = torch.ones(N + 2, dtype=torch.bool)
    rest[idx[visited]] = False
    assert not mean[:, rest].any() and not kw["x_out"][:, kw["order"][4:].long()].any()
    assert kw["partials"][0].item() == pytest.approx(kw["dn_out"][visited].double().sum().item(), rel=1e-12)
