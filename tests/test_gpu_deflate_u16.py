"""The 16-bit sample format of the device tile encoder on the GPU
(csrc/kf_deflate.hip: dfl_tile_dyn_kernel<DFL_FMT_U16, *>): bit-identical to
the host runner of the same source, decodable by the device TileDecoder, and
through KafkaOutput the same samples as the host encoder path."""
import datetime as dt
import functools

import numpy as np
import pytest
import torch

import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.input_output.tiff import read_tiff, tiff_info
from kafka_inferenceengine_amd.ops.kernels import TileDecoder, TileEncoder, ext, quantise_u16

H, W = 300, 260
RANGES = [(-0.37, 6.2), (0.0, 1.0), (0.5, 4.25)]


@functools.lru_cache(maxsize=None)
def _planes():
    """(3, 300, 260): a smooth plane, a constant plane (rows shorter than a
    word in both modes), and a plane with a NaN block and values outside its
    range, +-inf among them.  Partial tiles on both axes."""
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:H, 0:W]
    p = np.empty((3, H, W), np.float32)
    p[0] = 2.9 + 2.5 * np.sin(xx / 17.0) * np.cos(yy / 23.0) + 0.02 * rng.standard_normal((H, W))
    p[1] = 0.25
    p[2] = 2.4 + 2.2 * np.sin(xx / 29.0 + yy / 31.0) + 0.3 * rng.standard_normal((H, W))   # leaves [0.5, 4.25]
    p[2, 40:90, 100:180] = np.nan
    p[2, 270:, 250:] = np.nan
    p[2, 5, 3:9] = [np.inf, -np.inf, 1e30, -1e30, 0.5, 4.25]
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _host(mode):
    planes = torch.from_numpy(_planes().reshape(3, -1).copy())
    return TileEncoder(huffman=mode, sample="uint16").encode(planes, H, W, ranges=RANGES)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fixed", "dynamic"])
def test_device_uint16_encoder_bit_identical_to_host(cuda, mode):
    host = _host(mode)
    planes = torch.from_numpy(_planes().reshape(3, -1).copy()).to(cuda)
    dev = TileEncoder(huffman=mode, sample="uint16").encode(planes, H, W, ranges=RANGES)
    torch.cuda.synchronize()
    assert torch.equal(dev[1].cpu(), host[1]) and torch.equal(dev[2].cpu(), host[2])
    total = int(host[1].sum())
    assert torch.equal(dev[0][:total].cpu(), host[0][:total])
    assert dev[3].is_cuda and torch.equal(dev[3].cpu(), host[3])
    assert host[3][0] == 0 and host[3][1] == 0 and host[3][2] > 1000
    # a second call of the same encoder starts its counters at zero
    again = TileEncoder(huffman=mode, sample="uint16")
    again.encode(planes, H, W, ranges=RANGES)
    assert torch.equal(again.encode(planes, H, W, ranges=RANGES)[3].cpu(), host[3])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fixed", "dynamic"])
def test_device_encode_then_device_decode(cuda, mode):
    planes = torch.from_numpy(_planes().reshape(3, -1).copy()).to(cuda)
    packed, sizes, offs, _ = TileEncoder(huffman=mode, sample="uint16").encode(planes, H, W, ranges=RANGES)
    q, _ = quantise_u16(_planes(), RANGES)
    tx, ty = TileEncoder.tiles(H, W)
    per = tx * ty
    rc = torch.tensor([[t // tx, t % tx] for t in range(per)], dtype=torch.int32, device=cuda)
    dec = TileDecoder()
    for p in range(3):
        out = torch.zeros((H, W), dtype=torch.int16, device=cuda)
        sl = slice(p * per, (p + 1) * per)
        _, st = dec.decode(packed, offs[sl].contiguous(), sizes[sl].contiguous(), rc, elem_bytes=2, predictor=2,
                           window=(0, H, 0, W), out=out)
        torch.cuda.synchronize()
        assert (st.cpu() == int(ext().INF_OK)).all(), [TileDecoder.status_name(int(s)) for s in st.cpu()]
        assert np.array_equal(out.cpu().numpy().view(np.uint16), q[p])


@pytest.mark.gpu
def test_kafka_output_uint16_device_files_match_host_files(cuda, tmp_path):
    """Reference-cadence output as scaled 16-bit rasters: the device encoder's
    files (fixed and dynamic Huffman) hold, sample for sample, what the host
    encoder path of the same run writes, with the same tags and counters."""
    mask = np.ones((600, 520), bool)
    mask[::9] = False
    grid = [dt.datetime(2017, 1, 1) + dt.timedelta(days=16 * i) for i in range(4)]
    # narrow enough that some samples saturate
    ranges = {p: (0.05, 0.9) for p in k.TIP_PARAMETERS}
    ranges["TeLAI"] = (0.0, 3.0)
    unc = {p: (0.0, 0.5) for p in k.TIP_PARAMETERS}
    unc["TeLAI"] = (0.0, 6.0)

    def run(out):
        obs = k.SyntheticBHRObservations(mask, n_train=60, device=cuda, stream=False, n_pool=2, seed=1)
        kf = k.LinearKalman(obs, out, mask, k.create_nonlinear_observation_operator, k.TIP_PARAMETERS,
                            state_propagation=k.propagate_information_filter_LAI, device=cuda)
        kf.set_trajectory_uncertainty(np.array([0, 0, 0, 0, 0, 0, 0.04]))
        kf.run(grid, kf.state_from_prior(k.JRCPrior(k.TIP_PARAMETERS, mask)), None, None)
        torch.cuda.synchronize()

    stats = {}
    for name, kw in (("host", dict(encoder="host")), ("fixed", dict(encoder="device", huffman="fixed")),
                     ("dynamic", dict(encoder="device", huffman="dynamic"))):
        out = k.KafkaOutput(k.TIP_PARAMETERS, [0, 10, 0, 0, 0, -10], "EPSG:32630", str(tmp_path / name),
                            sample_type="uint16", ranges=ranges, unc_ranges=unc, **kw)
        run(out)
        out.flush()
        stats[name] = out.writer_stats()
        assert stats[name]["sample_type"] == "uint16" and "uint16" in stats[name]["deflate_backend"]
    assert stats["fixed"]["deflate_backend"].startswith("device")
    files = sorted(p.name for p in (tmp_path / "host").iterdir())
    assert len(files) == 3 * 14
    for name in ("fixed", "dynamic"):
        assert sorted(p.name for p in (tmp_path / name).iterdir()) == files
        assert stats[name]["raster_bytes"] == stats["host"]["raster_bytes"] == 3 * 14 * 600 * 520 * 2
        assert stats[name]["saturated"]["total"] == stats["host"]["saturated"]["total"] > 0
        assert sorted(stats[name]["saturated"]["last"].values()) == sorted(stats["host"]["saturated"]["last"].values())
        for fn in files:
            ref, _ = read_tiff(tmp_path / "host" / fn)
            arr, _ = read_tiff(tmp_path / name / fn)
            assert arr.dtype == np.uint16 and np.array_equal(arr, ref), (name, fn)
            a, b = tiff_info(tmp_path / name / fn), tiff_info(tmp_path / "host" / fn)
            assert all(a[key] == b[key] for key in ("dtype", "predictor", "nodata", "scale", "offset", "geotransform"))
    print(f"file bytes: fixed {stats['fixed']['file_bytes']}, dynamic {stats['dynamic']['file_bytes']}, "
          f"saturated {stats['fixed']['saturated']['total']}")
    assert stats["dynamic"]["file_bytes"] < stats["fixed"]["file_bytes"]
