"""SynergyKernels finds a date's band, uncertainty and mask files by editing the
file name only: a directory of the path that holds ``b0``, ``kernel_weights``
or ``mask`` must not be rewritten with it."""
import datetime as dt

import numpy as np

import kafka_inferenceengine_amd as k


def test_synergy_kernels_under_a_directory_named_like_a_band(tmp_path):
    shape = (3, 4)
    rng = np.random.default_rng(0)
    folder = tmp_path / "run_b0_kernel_weights" / "5b0175"
    folder.mkdir(parents=True)
    stem = folder / "Synergy.A2017010.h17v05"
    for b in range(7):
        k.write_tiff(f"{stem}_b{b}_kernel_weights.tif", rng.uniform(0.0, 0.3, (3, *shape)).astype(np.float32))
        k.write_tiff(f"{stem}_b{b}_kernel_unc.tif", np.full((3, *shape), 0.01, np.float32))
    m = np.ones(shape, np.uint8)
    m[1, 2] = 0
    k.write_tiff(f"{stem}mask.tif", m)
    obs = k.SynergyKernels(str(folder), "h17v05", dt.datetime(2017, 1, 5))
    assert obs.dates == [dt.datetime(2017, 1, 10)]
    for band in (0, 1):
        r = obs.get_band_data(obs.dates[0], band)
        assert not r.mask[1, 2] and r.mask.sum() == shape[0] * shape[1] - 1        # the mask file was found
        w = r.uncertainty.diagonal().reshape(shape)
        assert np.ptp(w[r.mask]) < 1e-6 * w[r.mask].max()                         # ... and the uncertainty files
