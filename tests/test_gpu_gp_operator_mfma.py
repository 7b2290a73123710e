"""``K.gp_operator(gp="mfma")`` (csrc/kf_gp_operator_mfma.hip) against the float64 emulator within the project's
gp_operator bound (tests/gp_operator_cases.py).  Measured on an MI355X, error over bound: value 0.33 at d = 2 (VALU
0.27; the NumPy twin of the sums alone, models/gp.py mfma_emulate, 0.21), below 0.2 elsewhere; gradient <= 0.10."""
import datetime as dt

import numpy as np
import pytest
import torch

import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.engine.bands import RecordCache
from kafka_inferenceengine_amd.ops import kernels as K

import gp_operator_cases as G
import kernel_cases as C
from test_gpu_aux import GP_OPERATOR_SHAPES, gp_operator_case, pad_untouched

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
RING_T = 32 * K.ext().gp_operator_resident_chunks(10) + 1   # the smallest 10-input table that leaves LDS
SHAPES = GP_OPERATOR_SHAPES + ((10, 4), "mixed")


def launch(n, tab, x0, N, pad):
    ldh = N + pad + 3
    h0, h = C.sentinel(2, ldh, DEV), C.sentinel(2 * n, ldh, DEV)
    K.gp_operator(n, tab, C.padded(x0.T, N + pad, DEV, fill=-777.0), h0, h, N=N, gp="mfma")
    assert pad_untouched(h0, N) and pad_untouched(h, N), (N, pad)
    return h0[:, :N].cpu().numpy(), h[:, :N].cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_shapes_vs_float64(shape):
    """Every (n, d) of the VALU kernel's test plus (10, 4) and one call with a d = 7 and a d = 4 band, at
    the C.aux_shape sizes: observed pixels inside the bound, masked pixels +0.0, padding untouched."""
    worst = [0.0, 0.0]
    for i in range(len(C.AUX_N)):
        N, pad = C.aux_shape(SHAPES.index(shape) + i)
        if shape in GP_OPERATOR_SHAPES:
            n, (x0, evals, table) = shape[0], gp_operator_case(*shape, N)
        else:
            n, maps = (10, G.MAPS_10_4) if shape == (10, 4) else (7, G.MAPS_7_MIXED)
            x0, evals, table = G.case(n, maps, N)
        h0, h = launch(n, table(DEV, pad), x0, N, pad)
        plan = K.LAST_GP_OPERATOR_PLAN
        assert plan["family"] == K.GP_OPERATOR_MFMA_KERNEL and len(plan["names"]) == (2 if shape == "mixed" else 1)
        worst = np.maximum(worst, G.errors(f"{shape} N={N}", evals, n, h0, h))
    assert worst[0] <= 1.0 and worst[1] <= 1.0, worst


@pytest.mark.parametrize("n,T,what", [(10, (RING_T, 64), "ring"), (4, (33, 32), "T = 33 and 32"),
                                      (7, (64, 64), "dark wave")])
def test_table_sizes_and_a_masked_wave(n, T, what):
    """A table past the resident LDS budget (the ring, one workgroup walking three pixel groups), T = 33 (two
    chunks, 31 padded points) beside T = 32, and a 64-pixel tile no lane of which observes the band."""
    N, pad = 257 + 256, 5
    x0, evals, table = G.case(n, (range(n),) * 2, N, T=T, dark=slice(64, 128) if what == "dark wave" else None)
    K.ext().set_max_blocks(2 if what == "ring" else 0)   # 2: one workgroup per band
    try:
        h0, h = launch(n, table(DEV, pad), x0, N, pad)
    finally:
        K.ext().set_max_blocks(0)
    assert K.LAST_GP_OPERATOR_PLAN["resident"] == [what != "ring", True]
    assert max(G.errors(what, evals, n, h0, h)) <= 1.0


def test_nan_input_poisons_its_own_pixel_only():
    n, N, pad = 7, 257 + 256, 64
    x0, evals, table = G.case(n, G.MAPS_7_MIXED, N)
    px = int(np.flatnonzero((evals[0][3][130:] > 0) & (evals[1][3][130:] > 0))[0]) + 130   # observed in both bands
    tab = table(DEV, pad)
    clean = launch(n, tab, x0, N, pad)
    x0[px, 0] = np.nan                       # state 0 feeds both bands
    bad = launch(n, tab, x0, N, pad)
    for a, b in zip(clean, bad):
        assert np.array_equal(np.delete(a, px, 1), np.delete(b, px, 1)) and np.isnan(b[:, px]).any()


def test_refusals_leave_the_valu_call_working():
    """CPU tensors, a linear band and a band without fragments: ValueError with gp="mfma"; the same call
    with gp="valu" runs (the linear band's on the host runner: the device's VALU kernels are GP-only)."""
    n, N, cpu = 4, 65, torch.device("cpu")
    x0, _, table = G.case(n, (range(n),) * 2, N)
    lin = C.nongp_case(n, N, (("gp", K.OBS_F32), ("linear", K.OBS_F32)))

    class NoFragments(RecordCache):
        def get_mfma(self, spec, device):
            return None

    for dev, vdev, tab_of in ((cpu, cpu, lambda d: table(d, 0)), (DEV, cpu, lambda d: C.nongp_table(lin, d, 0)[0]),
                              (DEV, DEV, lambda d: table(d, 0, NoFragments()))):
        with pytest.raises(ValueError, match="gp_operator\\(gp='mfma'\\)"):
            K.gp_operator(n, tab_of(dev), C.padded(x0.T, N, dev), C.sentinel(2, N, dev), C.sentinel(2 * n, N, dev),
                          N=N, gp="mfma")
        h0 = C.sentinel(2, N, vdev)
        K.gp_operator(n, tab_of(vdev), C.padded(x0.T, N, vdev), h0, C.sentinel(2 * n, N, vdev), N=N, d=n, gp="valu")
        assert torch.isfinite(h0).all() and bool((h0 != C.SENTINEL).all())


def test_engine_split_path_on_the_matrix_cores():
    """tests/test_engine.py test_split_gp_operator_path_equals_fused's problem and tolerances, mfma against valu."""
    mask = np.ones((10, 9), bool)
    obs = k.SyntheticS2Observations(mask, n_bands=10, n_train=30, device=DEV, stream=False, n_pool=2, field_cell=4)
    prior = k.SAILPrior(k.SAIL_PARAMETERS, mask)
    x0, Pinv = prior.process_prior(None)
    grid = [obs.dates[0] - dt.timedelta(days=1), obs.dates[1] + dt.timedelta(days=1)]
    res = []
    for gp in ("valu", "mfma"):
        K.LAST_GP_OPERATOR_PLAN = None
        kf = k.LinearKalman(obs, None, mask, k.create_prosail_observation_operator, k.SAIL_PARAMETERS,
                            state_propagation=None, prior=prior, device=DEV,
                            config=k.EngineConfig(gp_split="always", split_gp=gp, band_chunk=3))
        res.append((kf.run(grid, x0, None, Pinv), [h["gn_iterations"] for h in kf.history]))
        assert (K.LAST_GP_OPERATOR_PLAN is not None) == (gp == "mfma")
    assert K.LAST_GP_OPERATOR_PLAN["family"] == K.GP_OPERATOR_MFMA_KERNEL
    (a, ia), (b, ib) = res
    assert ia == ib and torch.allclose(a.x, b.x, rtol=1e-4, atol=1e-5)
    assert torch.allclose(a.P, b.P, rtol=1e-4, atol=1e-2)
