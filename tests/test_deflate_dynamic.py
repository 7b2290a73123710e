"""Dynamic-Huffman mode of the GeoTIFF tile encoder (csrc/kf_deflate.h,
ops.kernels.TileEncoder(huffman="dynamic")): the fixed mode's tokens under one
Huffman table per 256 x 256 tile, wherever that block is strictly smaller than
the fixed one.  Host runner here (the same shared source the gfx950 kernel
runs); the device streams are pinned bit-identical to it on the GPU."""
import datetime as dt
import functools
import hashlib
import zlib

import numpy as np
import pytest
import torch

import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.input_output.tiff import _read_tiff_py, read_tiff, tiff_info, write_tiff_tiles
from kafka_inferenceengine_amd.ops.kernels import TileEncoder, ext

# SHA-256 of the fixed-mode packed bytes, sizes and offsets (int64, little-endian)
# of _planes(2, 300, 520), computed on the commit before the dynamic mode
FIXED_SHA256 = "b738fd73c7b7fbaee47cf76c9d32acf86616dcb6f514e3c5d5e004e37f3f3392"


def _planes(n, H, W, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for i in range(n):
        f = np.sin(xx / (17.0 + i)) * np.cos(yy / 23.0) + 0.01 * rng.standard_normal((H, W))
        f[(yy // 40 + xx // 40) % 5 == 0] = 0.0           # flat patches: long runs
        out.append((f * (i + 1)).astype(np.float32))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def _tiles():
    """The test tiles (256 x 256 float32, read-only)."""
    yy, xx = np.mgrid[0:256, 0:256]
    a = (0.6 + 0.2 * np.sin(xx / 37.0) * np.cos(yy / 23.0)
         + 0.01 * np.random.default_rng(0).standard_normal((256, 256))).astype(np.float32)
    b = a.copy()
    b[:, :128] = 0.5
    const = np.full((256, 256), 0.5, np.float32)
    noise = np.random.default_rng(9).standard_normal((256, 256)).astype(np.float32)
    adv = np.where(xx % 2 == 0, 0.5, 0.75).astype(np.float32)
    adv[100] = np.random.default_rng(7).standard_normal(256).astype(np.float32)
    out = {"A": a, "B": b, "const": const, "noise": noise, "adv": adv}
    for v in out.values():
        v.setflags(write=False)
    return out


def _pred3_tile(plane, ty, tx):
    """Predictor-3 bytes of one zero-padded 256^2 tile (TIFF TN3, little-endian samples)."""
    t = np.zeros((256, 256), np.float32)
    blk = plane[ty * 256:(ty + 1) * 256, tx * 256:(tx + 1) * 256]
    t[:blk.shape[0], :blk.shape[1]] = blk
    b = t.view(np.uint8).reshape(256, 256, 4)[:, :, ::-1]          # MSB first
    rows = np.ascontiguousarray(b.transpose(0, 2, 1)).reshape(256, 1024)
    d = rows.copy()
    d[:, 1:] = (rows[:, 1:].astype(np.int16) - rows[:, :-1].astype(np.int16)).astype(np.uint8)
    return d.tobytes()


def _streams(planes, mode):
    """The host runner's streams of planes [n, H, W], one per tile."""
    E = ext()
    planes = np.ascontiguousarray(planes, np.float32)
    n, H, W = planes.shape
    tx, ty = TileEncoder.tiles(H, W)
    nt, bound = n * tx * ty, int(E.DFL_BOUND)
    out = np.zeros(nt * bound, np.uint8)
    sizes = np.zeros(nt, np.uint32)
    E.deflate_tiles(planes.ctypes.data, H * W, H, W, n, out.ctypes.data, sizes.ctypes.data, False, 0, 0,
                    {"fixed": E.DFL_MODE_FIXED, "dynamic": E.DFL_MODE_DYNAMIC,
                     "forced": E.DFL_MODE_DYNAMIC_FORCE_FIXED}[mode])
    return [out[i * bound:i * bound + int(sizes[i])].tobytes() for i in range(nt)]


@functools.lru_cache(maxsize=None)
def _tile_streams(name, mode):
    return _streams(_tiles()[name][None], mode)[0]


def _btype(stream):
    return (stream[2] >> 1) & 3


@pytest.mark.parametrize("name", ["A", "B", "const", "noise", "adv"])
def test_dynamic_stream_decodes_to_predicted_bytes(name):
    s = _tile_streams(name, "dynamic")
    assert s[:2] == b"\x78\x01" and s[2] & 1 == 1               # one final block
    assert zlib.decompress(s) == _pred3_tile(_tiles()[name], 0, 0)   # checks the Adler-32 too


def test_dynamic_padded_rasters_decode():
    H, W = 300, 520
    planes = _planes(2, H, W)
    tx, ty = TileEncoder.tiles(H, W)
    streams = _streams(planes, "dynamic")
    assert len(streams) == 2 * tx * ty
    for i, s in enumerate(streams):
        p, t = divmod(i, tx * ty)
        assert zlib.decompress(s) == _pred3_tile(planes[p], t // tx, t % tx), i


@pytest.mark.parametrize("name", ["A", "B", "noise", "adv"])
def test_dynamic_block_type(name):
    assert _btype(_tile_streams(name, "dynamic")) == 2
    assert _btype(_tile_streams(name, "fixed")) == 1


@pytest.mark.parametrize("name", ["A", "B", "const", "noise", "adv"])
def test_dynamic_never_larger_and_fallback_is_the_fixed_stream(name):
    fixed = _tile_streams(name, "fixed")
    assert len(_tile_streams(name, "dynamic")) <= len(fixed)
    # the dynamic path with the per-tile choice forced to the fixed block
    assert _tile_streams(name, "forced") == fixed


def test_fallback_on_padded_rasters_is_the_fixed_stream():
    planes = _planes(2, 300, 520)
    fixed, dyn = _streams(planes, "fixed"), _streams(planes, "dynamic")
    assert _streams(planes, "forced") == fixed
    assert all(len(d) <= len(f) for d, f in zip(dyn, fixed))


@pytest.mark.parametrize("name", ["A", "B", "noise"])
def test_dynamic_within_one_percent_of_zlib_rle(name):
    """Homogeneous tiles: one table per tile against zlib level 1 with Z_RLE
    (the same match family) on the same predicted bytes.  Tiles that mix noise
    rows with quiet rows are exempt: zlib re-plans its table per block there."""
    c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    raw = _pred3_tile(_tiles()[name], 0, 0)
    ref = len(c.compress(raw) + c.flush())
    got = len(_tile_streams(name, "dynamic"))
    print(f"{name}: dynamic {got} B, zlib level 1 Z_RLE {ref} B, ratio {got / ref:.4f}, "
          f"fixed {len(_tile_streams(name, 'fixed'))} B")
    assert got <= 1.01 * ref


def test_fixed_mode_bytes_unchanged():
    H, W = 300, 520
    planes = _planes(2, H, W)
    packed, sizes, offs = TileEncoder().encode(torch.from_numpy(planes.reshape(2, -1)), H, W)
    h = hashlib.sha256()
    h.update(packed.numpy()[:int(sizes.sum())].tobytes())
    h.update(sizes.numpy().astype("<i8").tobytes())
    h.update(offs.numpy().astype("<i8").tobytes())
    assert h.hexdigest() == FIXED_SHA256


def test_tile_encoder_dynamic_mode_packs_the_host_streams():
    H, W = 300, 520
    planes = _planes(2, H, W)
    packed, sizes, offs = TileEncoder(huffman="dynamic").encode(torch.from_numpy(planes.reshape(2, -1)), H, W)
    buf = packed.numpy().tobytes()
    got = [buf[int(o):int(o) + int(s)] for o, s in zip(offs, sizes)]
    assert got == _streams(planes, "dynamic")
    with pytest.raises(ValueError):
        TileEncoder(huffman="best")


def test_geotiff_from_dynamic_tiles_roundtrip(tmp_path):
    H, W = 300, 520
    planes = _planes(1, H, W, seed=3)
    packed, sizes, offs = TileEncoder(huffman="dynamic").encode(torch.from_numpy(planes.reshape(1, -1)), H, W)
    assert any(_btype(packed.numpy()[int(o):int(o) + 3].tobytes()) == 2 for o in offs)
    gt = [576452.58, 10.0, 0.0, 4324696.15, 0.0, -10.0]
    p = tmp_path / "lai_A2017001.tif"
    write_tiff_tiles(p, H, W, packed.numpy(), offs.numpy(), sizes.numpy(), gt, "EPSG:32630")
    a, info = read_tiff(p)
    assert np.array_equal(a, planes[0])
    assert info["geotransform"] == gt and info.get("epsg") == 32630
    b, _ = _read_tiff_py(p)                        # the independent Python decoder
    assert np.array_equal(b, planes[0])
    ti = tiff_info(p)
    assert ti["compression"] == 8 and ti["predictor"] == 3 and ti["tiled"] and ti["tile"] == (256, 256)


def test_kafka_output_rejects_dynamic_on_the_host_encoder(tmp_path):
    with pytest.raises(ValueError):
        k.KafkaOutput(k.TIP_PARAMETERS, [0, 10, 0, 0, 0, -10], "EPSG:32630", str(tmp_path), encoder="host",
                      huffman="dynamic")
    with pytest.raises(ValueError):
        k.KafkaOutput(k.TIP_PARAMETERS, [0, 10, 0, 0, 0, -10], "EPSG:32630", str(tmp_path), huffman="optimal")
    out = k.KafkaOutput(k.TIP_PARAMETERS, [0, 10, 0, 0, 0, -10], "EPSG:32630", str(tmp_path))
    assert out.huffman == "fixed"


def _gpu_planes():
    """(3, 300, 520): A over a _planes-style field, adv in an otherwise constant
    plane, a constant plane.  The adversarial tile is the first of its plane: a
    mistake in its rows' scratch lands in a following row of the same buffer."""
    H, W = 300, 520
    planes = np.empty((3, H, W), np.float32)
    planes[0] = _planes(1, H, W, seed=5)[0]
    planes[0, :256, :256] = _tiles()["A"]
    planes[1] = 0.25
    planes[1, :256, :256] = _tiles()["adv"]
    planes[2] = 0.5
    return planes


@pytest.mark.gpu
def test_device_dynamic_encoder_bit_identical_to_host(cuda):
    H, W = 300, 520
    planes = torch.from_numpy(_gpu_planes().reshape(3, -1))
    host = TileEncoder(huffman="dynamic").encode(planes, H, W)
    dev = TileEncoder(huffman="dynamic").encode(planes.to(cuda), H, W)
    torch.cuda.synchronize()
    assert torch.equal(dev[1].cpu(), host[1]) and torch.equal(dev[2].cpu(), host[2])
    total = int(host[1].sum())
    assert torch.equal(dev[0][:total].cpu(), host[0][:total])
    # the first tiles of planes 0 and 1 are dynamic blocks; the fixed mode is larger
    hb = host[0].numpy()
    tiles = H // 256 + 1, W // 256 + 1
    per = tiles[0] * tiles[1]
    assert _btype(hb[int(host[2][0]):][:3].tobytes()) == 2 and _btype(hb[int(host[2][per]):][:3].tobytes()) == 2
    fixed = TileEncoder().encode(planes.to(cuda), H, W)
    torch.cuda.synchronize()
    assert int(fixed[1].sum()) > total


@pytest.mark.gpu
def test_kafka_output_device_encoder_dynamic_files(cuda, tmp_path):
    """Reference-cadence output with the device encoder in the dynamic mode:
    every mean and uncertainty GeoTIFF decodes to the device rasters bit for
    bit, and the files are smaller than the fixed mode's."""
    mask = np.ones((600, 520), bool)
    mask[::9] = False
    grid = [dt.datetime(2017, 1, 1) + dt.timedelta(days=16 * i) for i in range(4)]

    def run(out):
        obs = k.SyntheticBHRObservations(mask, n_train=60, device=cuda, stream=False, n_pool=2, seed=1)
        kf = k.LinearKalman(obs, out, mask, k.create_nonlinear_observation_operator, k.TIP_PARAMETERS,
                            state_propagation=k.propagate_information_filter_LAI, device=cuda)
        kf.set_trajectory_uncertainty(np.array([0, 0, 0, 0, 0, 0, 0.04]))
        kf.run(grid, kf.state_from_prior(k.JRCPrior(k.TIP_PARAMETERS, mask)), None, None)
        torch.cuda.synchronize()

    ref = k.DeviceOutput(k.TIP_PARAMETERS, keep_history=True)
    run(ref)
    stats = {}
    for mode in ("fixed", "dynamic"):
        folder = tmp_path / mode
        out = k.KafkaOutput(k.TIP_PARAMETERS, [0, 10, 0, 0, 0, -10], "EPSG:32630", str(folder), encoder="device",
                            huffman=mode)
        run(out)
        out.flush()
        stats[mode] = out.writer_stats()
        assert stats[mode]["deflate_backend"].startswith("device") and mode in stats[mode]["deflate_backend"]
    for ts, (m, u) in ref.history.items():
        for p in range(7):
            name = f"{k.TIP_PARAMETERS[p]}_{ts.strftime('A%Y%j')}"
            assert np.array_equal(read_tiff(tmp_path / "dynamic" / f"{name}.tif")[0].reshape(-1), m[p].cpu().numpy())
            assert np.array_equal(read_tiff(tmp_path / "dynamic" / f"{name}_unc.tif")[0].reshape(-1),
                                  u[p].cpu().numpy())
    print(f"file bytes: fixed {stats['fixed']['file_bytes']}, dynamic {stats['dynamic']['file_bytes']}")
    assert stats["dynamic"]["file_bytes"] < stats["fixed"]["file_bytes"]
