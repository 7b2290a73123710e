"""The GeoTIFF tile decoder (csrc/kf_inflate.h, ops.kernels.TileDecoder) on the
host runner: the source the gfx950 kernel runs.  Oracle: zlib / numpy, compared
for bit equality.  The device pins itself to this in tests/test_gpu_inflate.py."""
import zlib

import numpy as np
import pytest
import torch

import inflate_cases as C
from kafka_inferenceengine_amd.input_output.streaming import RasterIngest
from kafka_inferenceengine_amd.input_output.tiff import read_tiff_window, write_tiff
from kafka_inferenceengine_amd.ops.kernels import TileDecoder, ext

T = C.T
WINDOWS = [(0, 300, 0, 520), (40, 200, 270, 500), (100, 300, 130, 520)]   # full; inside tile (0, 1); across all


def test_corpus_has_every_block_type():
    types = {C.btype(s) for _, s, _ in C.corpus16()}
    assert types == {0, 1, 2}
    for huffman, want in (("fixed", 1), ("dynamic", 2)):
        packed, sizes, offs, _ = C.encoder_streams(huffman)
        first = {C.btype(bytes(packed[int(o):int(o) + 3].numpy())) for o in offs}
        assert want in first


def test_corpus_decodes_to_the_raw_bytes():
    cases = C.corpus16()
    for lo in range(0, len(cases), 20):
        part = cases[lo:lo + 20]
        got, status = C.decode_raw([s for _, s, _ in part])
        assert not status.any(), [(n, C.status_names()[v]) for (n, _, _), v in zip(part, status) if v]
        for (name, s, raw), g in zip(part, got):
            assert zlib.decompress(s) == raw
            assert g.tobytes() == raw, name


@pytest.mark.parametrize("huffman", ["fixed", "dynamic"])
def test_own_encoder_streams_round_trip(huffman):
    """TileEncoder (CPU) -> TileDecoder with predictor 3: the input's bits; the
    tiles' padding is never written."""
    packed, sizes, offs, rc = C.encoder_streams(huffman)
    planes = C.float_planes()
    for p in range(2):
        sel = slice(6 * p, 6 * p + 6)
        out = torch.full((300, 520), 7.0)
        _, st = TileDecoder().decode(packed, offs[sel].contiguous(), sizes[sel].contiguous(), rc[sel].contiguous(),
                                     elem_bytes=4, predictor=3, window=(0, 300, 0, 520), out=out)
        assert not st.any() and st.numel() == 6
        assert np.array_equal(out.numpy().view(np.uint32), planes[p].view(np.uint32))


def _pred2_stream(tile16):
    d = tile16.copy()
    d[:, 1:] = tile16[:, 1:] - tile16[:, :-1]
    return zlib.compress(d.tobytes(), 6)


def _pred3_stream(tile32):
    b = tile32.view(np.uint8).reshape(T, T, 4)[:, :, ::-1]
    rows = np.ascontiguousarray(b.transpose(0, 2, 1)).reshape(T, 4 * T)
    d = rows.copy()
    d[:, 1:] = rows[:, 1:] - rows[:, :-1]
    return zlib.compress(d.tobytes(), 6)


def test_predictor_undo_against_numpy():
    rng = np.random.default_rng(3)
    t16 = rng.integers(0, 65536, (T, T), dtype=np.uint16)
    t16[50:60] = 65535
    data, offs, sizes = C.pack([_pred2_stream(t16)])
    rc = torch.zeros((1, 2), dtype=torch.int32)
    out = torch.zeros((T, T), dtype=torch.int16)
    _, st = TileDecoder().decode(data, offs, sizes, rc, elem_bytes=2, predictor=2, window=(0, T, 0, T), out=out)
    assert not st.any()
    assert np.array_equal(out.numpy().view(np.uint16), t16)
    t32 = rng.standard_normal((T, T)).astype(np.float32)
    t32[7, 9] = np.nan
    data, offs, sizes = C.pack([_pred3_stream(t32)])
    out = torch.zeros((T, T), dtype=torch.float32)
    _, st = TileDecoder().decode(data, offs, sizes, rc, elem_bytes=4, predictor=3, window=(0, T, 0, T), out=out)
    assert not st.any()
    assert np.array_equal(out.numpy().view(np.uint32), t32.view(np.uint32))


@pytest.fixture(scope="module")
def raster(tmp_path_factory):
    """The 300 x 520 uint16 raster (2 x 3 tiles with ragged edges) as predictor-1 and predictor-2 files."""
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:300, 0:520]
    a = (2000 + 900 * np.sin(xx / 29.0) * np.cos(yy / 13.0) + rng.normal(0, 9, (300, 520))).astype(np.uint16)
    a[120:140, 200:300] = 0
    d = tmp_path_factory.mktemp("inflate")
    paths = {}
    for pred in (1, 2):
        paths[pred] = str(d / f"p{pred}.tif")
        write_tiff(paths[pred], a, predictor=pred)
    return a, paths


@pytest.mark.parametrize("pred", [1, 2])
@pytest.mark.parametrize("win", WINDOWS)
def test_window_placement_matches_the_host_reader(raster, pred, win):
    a, paths = raster
    r0, r1, c0, c1 = win
    t = ext().tiff_tile_table(paths[pred], 0, *win)
    assert t["tile"] == 256 and t["predictor"] == pred and t["compression"] == 8 and t["bits"] == 16
    with open(paths[pred], "rb") as f:
        blob = f.read()
    data, offs, sizes = C.pack([blob[o:o + n] for o, n in zip(t["offsets"], t["counts"])])
    rc = torch.tensor(t["tile_rc"], dtype=torch.int32).view(-1, 2)
    # the destination is wider than the window: the sentinel around it must survive
    full = torch.full((r1 - r0 + 2, c1 - c0 + 5), 21845, dtype=torch.int16)
    out = full[1:-1, 2:2 + c1 - c0]
    _, st = TileDecoder().decode(data, offs, sizes, rc, elem_bytes=2, predictor=pred, window=win, out=out)
    assert not st.any() and st.numel() == len(t["offsets"])
    want = read_tiff_window(paths[pred], 0, win)
    assert np.array_equal(want, a[r0:r1, c0:c1])
    assert np.array_equal(out.numpy().view(np.uint16), want)
    border = full.clone()
    border[1:-1, 2:2 + c1 - c0] = 21845
    assert bool((border == 21845).all()) and bool((full[0] == 21845).all()) and bool((full[:, :2] == 21845).all())


@pytest.mark.parametrize("pred", [1, 2])
def test_raster_ingest_device_decoder_on_cpu(raster, pred):
    """RasterIngest(decoder="device") on the CPU device runs the host runner of the decoder, not the host reader."""
    a, paths = raster
    for win in WINDOWS:
        r0, r1, c0, c1 = win
        files = [(paths[pred], 0, win)]
        planes = {}
        for mode in ("host", "device"):
            ing = RasterIngest(1, (r1 - r0, c1 - c0), torch.int16, "cpu", decoder=mode)
            planes[mode] = ing.acquire("d", files).clone()
            ing.check()
            if mode == "device":
                st = ing.stats()
                ntiles = len(ext().tiff_tile_table(paths[pred], 0, *win)["offsets"])
                assert st["files_host"] == 0 and st["files_device"] == 1 and st["tiles_device"] == ntiles
                assert st["bytes_compressed_h2d"] > 0 and st["bytes_raw"] == (r1 - r0) * (c1 - c0) * 2
                assert ing.bytes_h2d < 24 * ntiles + 16 + st["bytes_compressed_h2d"] + 1
        assert torch.equal(planes["host"], planes["device"])
        assert np.array_equal(planes["device"][0].numpy().view(np.uint16), a[r0:r1, c0:c1])


def test_raster_ingest_falls_back_per_file(raster, tmp_path):
    """Striped, uncompressed and 128-pixel-tile files take the host reader, counted per file."""
    a, paths = raster
    others = {"striped": dict(tile=None), "raw": dict(compress=None), "tile128": dict(tile=128)}
    files = [(paths[1], 0, (0, 300, 0, 520))]
    for name, kw in others.items():
        p = str(tmp_path / f"{name}.tif")
        write_tiff(p, a, **kw)
        files.append((p, 0, (0, 300, 0, 520)))
    ing = RasterIngest(len(files), (300, 520), torch.int16, "cpu", decoder="device")
    planes = ing.acquire("d", files)
    ing.check()
    st = ing.stats()
    assert st["files_device"] == 1 and st["files_host"] == 3 and st["tiles_device"] == 6
    for i in range(len(files)):
        assert np.array_equal(planes[i].numpy().view(np.uint16), a)


def test_raster_ingest_reports_a_broken_tile(raster, tmp_path):
    a, paths = raster
    t = ext().tiff_tile_table(paths[1], 0, 0, 300, 0, 520)
    blob = bytearray(open(paths[1], "rb").read())
    o, n = t["offsets"][4], t["counts"][4]
    blob[o + 2:o + n] = bytes(n - 2)
    p = str(tmp_path / "broken.tif")
    open(p, "wb").write(bytes(blob))
    ing = RasterIngest(1, (300, 520), torch.int16, "cpu", decoder="device")
    with pytest.raises(RuntimeError, match=r"broken\.tif: tile \(row 1, column 1\): INF_"):
        ing.acquire("d", [(p, 0, (0, 300, 0, 520))])
        ing.check()
    got = ing.bufs[0][0].numpy().view(np.uint16)
    assert not got[256:300, 256:512].any()                      # the failed tile reads as no observation
    assert np.array_equal(got[:256], a[:256])


# ---------------------------------------------------------------- malformed input
def _run_malformed(cases):
    """-> {name: (status, tile bytes)} of malformed cases, grouped by raw size."""
    out = {}
    by_raw = {}
    for c in cases:
        by_raw.setdefault(c[2], []).append(c)
    dec = TileDecoder()
    for raw_bytes, group in by_raw.items():
        for lo in range(0, len(group), 128):
            part = group[lo:lo + 128]
            got, status = C.decode_raw([c[1] for c in part], raw_bytes=raw_bytes, decoder=dec)
            for c, g, s in zip(part, got, status):
                out[c[0]] = (int(s), g)
    return out


def test_malformed_streams_end_in_a_status_and_a_zeroed_tile():
    cases = C.malformed()
    assert len(cases) > 800
    res = _run_malformed(cases)
    names = C.status_names()
    seen = set()
    for name, stream, raw_bytes, tile in cases:
        status, got = res[name]
        if name.startswith("flip") and raw_bytes == C.RAW16 and C.zlib_verdict(stream, tile):
            assert status == 0 and got.tobytes() == tile, name     # zlib decodes it to the right bytes: so do we
            continue
        assert status != 0, name
        assert not got.any(), (name, names[status])
        seen.add(names[status])
    for name in C.GPU_MALFORMED:                                   # the device test's list: each returns a status here
        assert res[name][0] != 0, name
    assert {"INF_TRUNCATED", "INF_BAD_HEADER", "INF_BAD_BLOCK", "INF_BAD_STORED", "INF_BAD_ADLER", "INF_OVERRUN",
            "INF_SHORT"} <= seen, seen


def test_ranges_outside_the_buffer_are_truncated():
    s, tile = C.small_dynamic()
    data, offs, sizes = C.pack([s, s])
    sizes[1] += 1                                                  # one byte past the end of data
    rc = torch.tensor([[0, 0], [1, 0]], dtype=torch.int32)
    out = torch.full((2 * T, T), 21845, dtype=torch.int16)
    _, st = TileDecoder().decode(data, offs, sizes, rc, elem_bytes=2, window=(0, 2 * T, 0, T), out=out)
    assert st.tolist() == [0, C.status_names().index("INF_TRUNCATED")]
    assert out[:T].numpy().tobytes() == tile and not out[T:].any()


def test_unsupported_layouts_are_refused():
    data, offs, sizes = C.pack([C.small_dynamic()[0]])
    rc = torch.zeros((1, 2), dtype=torch.int32)
    out = torch.zeros((T, T), dtype=torch.int16)
    with pytest.raises(ValueError):
        TileDecoder().decode(data, offs, sizes, rc, tile=128, elem_bytes=2, window=(0, T, 0, T), out=out)
    with pytest.raises(ValueError):
        TileDecoder().decode(data, offs, sizes, rc, elem_bytes=2, predictor=3, window=(0, T, 0, T), out=out)
