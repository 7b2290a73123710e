"""The device GeoTIFF tile decoder (csrc/kf_inflate.hip: inf_tile_kernel) on
the MI355X, pinned bit for bit to the host runner of the same source
(tests/test_inflate.py pins that to zlib / numpy), and the ingest path built
on it (RasterIngest / Sentinel2Observations with decoder="device")."""
import datetime as dt
import glob
import os

import numpy as np
import pytest
import torch

import inflate_cases as C
import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.input_output import sentinel as S
from kafka_inferenceengine_amd.input_output.streaming import RasterIngest
from kafka_inferenceengine_amd.input_output.tiff import write_tiff
from kafka_inferenceengine_amd.ops.kernels import TileDecoder, ext

pytestmark = pytest.mark.gpu
T = C.T
WINDOWS = [(0, 300, 0, 520), (40, 200, 270, 500), (100, 300, 130, 520)]


def test_corpus_equals_the_host_runner():
    cases = C.corpus16()
    assert len(cases) == 40
    streams = [s for _, s, _ in cases]
    got, status = C.decode_raw(streams, device="cuda")
    ref, ref_status = C.decode_raw(streams)
    assert not status.any() and np.array_equal(status, ref_status)
    assert np.array_equal(got, ref)
    for (name, _, raw), g in zip(cases, got):
        assert g.tobytes() == raw, name


@pytest.mark.parametrize("huffman", ["fixed", "dynamic"])
def test_encode_decode_round_trip_on_the_device(huffman):
    packed, sizes, offs, rc = C.encoder_streams(huffman, device="cuda")
    planes = C.float_planes()
    dec = TileDecoder()
    for p in range(2):
        sel = slice(6 * p, 6 * p + 6)
        out = torch.full((300, 520), 7.0, device="cuda")
        _, st = dec.decode(packed, offs[sel].contiguous(), sizes[sel].contiguous(), rc[sel].contiguous(),
                           elem_bytes=4, predictor=3, window=(0, 300, 0, 520), out=out)
        assert st.numel() == 6 and not st.cpu().any()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), planes[p].view(np.uint32))


@pytest.fixture(scope="module")
def raster(tmp_path_factory):
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:300, 0:520]
    a = (2000 + 900 * np.sin(xx / 29.0) * np.cos(yy / 13.0) + rng.normal(0, 9, (300, 520))).astype(np.uint16)
    a[120:140, 200:300] = 0
    d = tmp_path_factory.mktemp("gpu_inflate")
    paths = {}
    for pred in (1, 2):
        paths[pred] = str(d / f"p{pred}.tif")
        write_tiff(paths[pred], a, predictor=pred)
    return a, paths


@pytest.mark.parametrize("pred", [1, 2])
def test_raster_ingest_device_equals_host(raster, pred):
    a, paths = raster
    for win in WINDOWS:
        r0, r1, c0, c1 = win
        files = [(paths[pred], 0, win)]
        planes = {}
        for mode in ("host", "device"):
            ing = RasterIngest(1, (r1 - r0, c1 - c0), torch.int16, "cuda", decoder=mode)
            planes[mode] = ing.acquire("d", files).clone()
            torch.cuda.synchronize()
            ing.check()
            if mode == "device":
                st = ing.stats()
                ntiles = len(ext().tiff_tile_table(paths[pred], 0, *win)["offsets"])
                assert st["files_host"] == 0 and st["files_device"] == 1 and st["tiles_device"] == ntiles
        assert torch.equal(planes["host"], planes["device"])
        assert np.array_equal(planes["device"][0].cpu().numpy().view(np.uint16), a[r0:r1, c0:c1])


def test_malformed_streams_beside_valid_ones():
    """12 malformed streams (each returns a status on the host runner:
    tests/test_inflate.py) in one launch beside 4 valid ones."""
    by_name = {c[0]: c for c in C.malformed()}
    bad = [by_name[n] for n in C.GPU_MALFORMED]
    assert len(bad) == 12 and all(c[2] == C.RAW16 for c in bad)
    good = [c for c in C.corpus16() if c[0] in ("smooth-l6", "random-l0", "repeat-l9", "geometric-fixed")]
    assert len(good) == 4
    streams = [good[0][1]] + [c[1] for c in bad[:6]] + [good[1][1], good[2][1]] + [c[1] for c in bad[6:]] + [good[3][1]]
    where = [0, 7, 8, 15]
    got, status = C.decode_raw(streams, device="cuda")
    ref, ref_status = C.decode_raw(streams)
    assert np.array_equal(status, ref_status)
    for i in range(16):
        if i in where:
            assert status[i] == 0 and got[i].tobytes() == good[where.index(i)][2]
        else:
            assert status[i] != 0 and not got[i].any()
    assert np.array_equal(got, ref)


def _archive(root, dates, seed, emus):
    rng = np.random.default_rng(seed)
    mu, _, _ = k.sail_prior()
    dn_by_date = {}
    for d in dates:
        # a 64 x 64 block of emulator-consistent reflectances (the Gauss-Newton loop converges), repeated 8 x 8
        truth = mu[None, :] + rng.normal(0, 0.03, (64 * 64, mu.size))
        two = [np.tile(np.round(np.clip(emus[b].predict(truth)[0].reshape(64, 64) + rng.normal(0, 0.002, (64, 64)),
                                        0.01, 0.8) * 1e4).astype(np.uint16), (8, 8)) for b in range(2)]
        two[0][:5, :7] = 0
        dn_by_date[d] = np.stack([two[i % 2] for i in range(10)])
    keys = {f"S2A_MSI_{S.S2_EMULATOR_BANDS[b]:02d}": emus[b] for b in range(10)}
    return S.write_s2_archive(str(root), dn_by_date, keys)


def _run(data, emu, decoder, out_dir, device="cuda"):
    mask = np.ones((512, 512), bool)
    obs = S.Sentinel2Observations(data, emu, mask, decoder=decoder)
    obs.band_map = obs.band_map[:2]                     # a 2-band date
    obs.bands_per_observation = {d: 2 for d in obs.dates}
    prior = k.SAILPrior(k.SAIL_PARAMETERS, mask)
    out = k.KafkaOutput(k.SAIL_PARAMETERS, None, "", str(out_dir), encoder="host")
    kf = k.LinearKalman(obs, out, mask, k.create_prosail_observation_operator, k.SAIL_PARAMETERS,
                        state_propagation=None, prior=prior, device=device)
    x0, Pinv = prior.process_prior(None)
    grid = [obs.dates[0] - dt.timedelta(days=1)] + [d + dt.timedelta(days=1) for d in obs.dates]
    st = kf.run(grid, x0, None, Pinv)
    out.flush()
    obs.check()
    return st.x.cpu().numpy().copy(), obs


def test_s2_archive_through_the_engine(tmp_path):
    dates = [dt.datetime(2017, 7, 3) + dt.timedelta(days=2 * i) for i in range(4)]
    emus = k.make_prosail_emulators(10, n_train=40)
    data, emu = _archive(tmp_path / "a", dates, 2, emus)
    xs, files = {}, {}
    for mode in ("host", "device"):
        xs[mode], obs = _run(data, emu, mode, tmp_path / mode)
        files[mode] = sorted(os.path.basename(p) for p in glob.glob(str(tmp_path / mode / "*.tif")))
        if mode == "device":
            st = obs.ingest_stats()
            assert st["files_host"] == 0 and st["files_device"] == 4 * 2 and st["tiles_device"] == 4 * 2 * 4
            assert 0 < st["bytes_compressed_h2d"] < st["bytes_raw"] == 4 * 2 * 512 * 512 * 2
    assert np.array_equal(xs["host"].view(np.uint32), xs["device"].view(np.uint32))
    assert files["host"] == files["device"] and len(files["host"]) > 0
    for f in files["host"]:
        assert open(tmp_path / "host" / f, "rb").read() == open(tmp_path / "device" / f, "rb").read(), f
    # a fifth archive with one tile's bytes overwritten: run raises
    data5, emu5 = _archive(tmp_path / "b", dates[:1], 3, emus)
    victim = glob.glob(os.path.join(data5, "**", "B03_sur.tif"), recursive=True)[0]
    t = ext().tiff_tile_table(victim, 0, 0, 512, 0, 512)
    blob = bytearray(open(victim, "rb").read())
    o, n = t["offsets"][3], t["counts"][3]
    blob[o + 2:o + n] = bytes(n - 2)
    open(victim, "wb").write(bytes(blob))
    with pytest.raises(RuntimeError, match=r"B03_sur\.tif: tile \(row 1, column 1\): INF_"):
        _run(data5, emu5, "device", tmp_path / "broken")
