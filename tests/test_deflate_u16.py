"""Scaled 16-bit output rasters (csrc/kf_deflate.h: dfl_quantise, DFL_FMT_U16;
ops.kernels.TileEncoder(sample="uint16")): the float planes are quantised in
the encoder's row load and written under TIFF predictor 2, 512 predicted bytes
per tile row.  Host runner here (the shared source the gfx950 kernels run); the
device streams are pinned bit-identical to it in tests/test_gpu_deflate_u16.py.

The adversarial tile: the issue asks for rows holding runs of exactly 258, 259
and 516 equal bytes.  A 16-bit tile row is 512 bytes and every row is
tokenised on its own, so 516 cannot occur; its place is taken by the two
longest cases a row can hold: 260 (a full 258-run that goes on) and the whole
row of 512 equal bytes (1 literal + 258 + 253)."""
import functools
import json
import zlib

import numpy as np
import pytest
import torch

import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.input_output.tiff import (_read_tiff_py, _write_tiff_py, read_tiff, read_tiff_scaled,
                                                         tiff_info, write_tiff, write_tiff_tiles)
from kafka_inferenceengine_amd.ops.kernels import TileEncoder, ext, quantise_u16

RAW16 = 256 * 256 * 2
LO, HI = -0.37, 6.2


def _values(q, lo=LO, hi=HI):
    """float32 values that quantise to the samples q (asserted where used)."""
    return (lo + (hi - lo) / 65534.0 * q.astype(np.float64)).astype(np.float32)


def _adv_samples():
    """uint16 samples of the adversarial tile: alternating 0 / 65534 columns
    (differences 65534 and 2: wrap-around), and four rows whose predicted bytes
    start with 258, 259, 260 and 512 equal bytes."""
    q = np.zeros((256, 256), np.uint16)
    q[:, 1::2] = 65534
    for row, run in ((10, 258), (11, 259), (12, 260), (13, 512)):
        b = np.empty(512, np.uint8)
        b[:run] = 2
        i = np.arange(512 - run)
        b[run:] = np.where(i % 2 == 0, 4 + 2 * (i // 2 % 50), 0)   # low bytes vary, high bytes 0: no long run
        b[run:run + 1] = 6                                         # the run ends exactly at `run`
        q[row] = np.cumsum(b.view("<u2"), dtype=np.uint16)
    assert q.max() <= 65534
    return q


def _runs(b):
    """lengths of the runs of equal bytes of a row"""
    edges = np.flatnonzero(np.diff(b.astype(np.int16)) != 0)
    return np.diff(np.concatenate([[-1], edges, [len(b) - 1]]))


@functools.lru_cache(maxsize=None)
def _rasters():
    """name -> (planes [n, H, W] float32, ranges); read-only."""
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:256, 0:256]
    smooth = (2.9 + 2.5 * np.sin(xx / 37.0) * np.cos(yy / 23.0) + 0.02 * rng.standard_normal((256, 256)))
    nan = smooth.copy()
    nan[40:90, 100:180] = np.nan
    yy, xx = np.mgrid[0:300, 0:260]
    padded = 2.9 + 2.5 * np.sin(xx / 17.0) * np.cos(yy / 23.0) + 0.02 * rng.standard_normal((300, 260))
    padded[(yy // 40 + xx // 40) % 5 == 0] = 0.0
    out = {
        "smooth": smooth[None],
        "const": np.full((1, 256, 256), 1.25),
        "noise": rng.uniform(LO, HI, (1, 256, 256)),
        "adv": _values(_adv_samples())[None],
        "nan": nan[None],
        "padded": np.stack([padded, 0.5 * padded + 1.0]),
        "one": np.full((1, 1, 1), 3.0),
    }
    out = {name: np.ascontiguousarray(v, np.float32) for name, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


NAMES = ["smooth", "const", "noise", "adv", "nan", "padded", "one"]


def _ranges(planes):
    return [(LO, HI)] * planes.shape[0]


def _streams(planes, mode, ranges=None):
    """The host runner's 16-bit streams of planes [n, H, W], one per tile, and the saturation counts."""
    E = ext()
    planes = np.ascontiguousarray(planes, np.float32)
    n, H, W = planes.shape
    a, b, _, _ = TileEncoder.quantiser(ranges or _ranges(planes))
    tx, ty = TileEncoder.tiles(H, W)
    nt, bound = n * tx * ty, int(E.DFL_BOUND16)
    out = np.zeros(nt * bound, np.uint8)
    sizes = np.zeros(nt, np.uint32)
    sat = np.zeros(n, np.uint32)
    E.deflate_tiles(planes.ctypes.data, H * W, H, W, n, out.ctypes.data, sizes.ctypes.data, False, 0, 0,
                    {"fixed": E.DFL_MODE_FIXED, "dynamic": E.DFL_MODE_DYNAMIC,
                     "forced": E.DFL_MODE_DYNAMIC_FORCE_FIXED}[mode], E.DFL_FMT_U16, a.ctypes.data, b.ctypes.data,
                    sat.ctypes.data)
    return [out[i * bound:i * bound + int(sizes[i])].tobytes() for i in range(nt)], sat


@functools.lru_cache(maxsize=None)
def _named_streams(name, mode):
    return _streams(_rasters()[name], mode)


def _pred2_tile(q, ty, tx):
    """Predictor-2 bytes of one zero-padded 256^2 tile of uint16 samples (little-endian)."""
    t = np.zeros((256, 256), np.uint16)
    blk = q[ty * 256:(ty + 1) * 256, tx * 256:(tx + 1) * 256]
    t[:blk.shape[0], :blk.shape[1]] = blk
    d = t.copy()
    d[:, 1:] = t[:, 1:] - t[:, :-1]                 # mod 65536
    return d.astype("<u2").tobytes()


# ------------------------------------------------------------------ quantiser
def _model_inputs():
    rng = np.random.default_rng(11)
    span = HI - LO
    v = rng.uniform(LO - 0.1 * span, HI + 0.1 * span, (300, 260)).astype(np.float32)
    v[0, :8] = [np.nan, np.inf, -np.inf, 1e30, -1e30, LO, HI, 0.0]
    v[5:9, 7:30] = np.nan
    t64 = (v.astype(np.float64) - LO) * 65534.0 / span
    with np.errstate(invalid="ignore"):
        near = (np.abs(t64 + 0.5) < 0.05) | (np.abs(t64 - 65534.5) < 0.05)
    v[near] = LO                                   # t64 = 0: far from both ends
    return v


def test_quantiser_against_float64_model():
    v = _model_inputs()
    span = HI - LO
    q, sat = quantise_u16(v[None], [(LO, HI)])
    q = q[0].astype(np.int64)
    _, _, scale, offset = TileEncoder.quantiser([(LO, HI)])
    assert scale[0] == span / 65534.0 and offset[0] == LO
    nan = np.isnan(v)
    t64 = (v.astype(np.float64) - LO) * 65534.0 / span
    with np.errstate(invalid="ignore"):
        # the count is unambiguous by the reference alone: nothing near the two ends
        assert not ((np.abs(t64 + 0.5) < 0.05) | (np.abs(t64 - 65534.5) < 0.05)).any()
        r = np.rint(t64)
        ref = np.where(nan, 65535, np.clip(r, 0, 65534))
        saturated = ~nan & ((r < 0) | (r > 65534))
    assert nan.sum() > 50 and saturated.sum() > 1000
    assert (q[nan] == 65535).all() and (q[~nan] <= 65534).all()
    assert np.abs(q - ref).max() <= 1
    assert q[0, 1] == 65534 and q[0, 2] == 0 and q[0, 3] == 65534 and q[0, 4] == 0      # +-inf, +-1e30
    assert q[0, 5] == 0 and q[0, 6] == 65534
    inr = ~nan & (v.astype(np.float64) >= LO) & (v.astype(np.float64) <= HI)
    err = np.abs(offset[0] + scale[0] * q[inr] - v[inr].astype(np.float64))
    print(f"decoded error: max {err.max() / scale[0]:.4f} scale")
    assert err.max() <= 0.52 * scale[0]
    assert int(sat[0]) == int(saturated.sum())
    # the encoder counts the same, in both modes, once per sample
    for mode in ("fixed", "dynamic"):
        assert int(_streams(v[None], mode)[1][0]) == int(saturated.sum())


def test_quantiser_rejects_bad_ranges():
    for rg in ((1.0, 1.0), (2.0, 1.0), (0.0, np.inf), (np.nan, 1.0)):
        with pytest.raises(ValueError):
            TileEncoder.quantiser([rg])
    enc = TileEncoder(sample="uint16")
    planes = torch.zeros((1, 4))
    with pytest.raises(ValueError):
        enc.encode(planes, 2, 2)                                  # ranges are required
    with pytest.raises(ValueError):
        enc.encode(planes, 2, 2, ranges=[(0, 1), (0, 1)])         # one per plane
    with pytest.raises(ValueError):
        TileEncoder().encode(planes, 2, 2, ranges=[(0, 1)])       # float32 takes none
    with pytest.raises(ValueError):
        TileEncoder(sample="int16")


def test_adversarial_tile_is_what_it_says():
    planes = _rasters()["adv"]
    q = quantise_u16(planes, _ranges(planes))[0][0]
    assert np.array_equal(q, _adv_samples())
    rows = np.frombuffer(_pred2_tile(q, 0, 0), np.uint8).reshape(256, 512)
    assert {65534, 2} <= set(np.frombuffer(rows[0].tobytes(), "<u2").tolist())      # wrap-around differences
    for row, run in ((10, 258), (11, 259), (12, 260), (13, 512)):
        assert _runs(rows[row])[0] == run


# -------------------------------------------------------------------- streams
@pytest.mark.parametrize("mode", ["fixed", "dynamic"])
@pytest.mark.parametrize("name", NAMES)
def test_streams_inflate_to_predictor2_bytes(name, mode):
    planes = _rasters()[name]
    n, H, W = planes.shape
    q, sat = quantise_u16(planes, _ranges(planes))
    streams, esat = _named_streams(name, mode)
    tx, ty = TileEncoder.tiles(H, W)
    assert len(streams) == n * tx * ty
    for i, s in enumerate(streams):
        p, t = divmod(i, tx * ty)
        raw = zlib.decompress(s)                    # zlib checks the Adler-32
        assert len(raw) == RAW16
        assert raw == _pred2_tile(q[p], t // tx, t % tx), (name, mode, i)
    assert np.array_equal(esat.astype(np.int64), sat)
    if name == "nan":
        assert (q[0][40:90, 100:180] == 65535).all()


def test_constant_rows_are_shorter_than_a_word_pair():
    """A constant 16-bit row is one literal and two matches: under 64 bits in
    both modes, the case the float32 fixed-mode merge cannot take."""
    for mode in ("fixed", "dynamic"):
        s = _named_streams("const", mode)[0][0]
        assert (len(s) - 6) * 8 / 256 < 64


@pytest.mark.parametrize("name", NAMES)
def test_dynamic_never_larger_and_forced_is_fixed(name):
    fx, dy, ff = (_named_streams(name, m)[0] for m in ("fixed", "dynamic", "forced"))
    assert all(len(d) <= len(f) for d, f in zip(dy, fx))
    assert ff == fx
    if name in ("smooth", "noise", "padded"):
        assert sum(map(len, dy)) < sum(map(len, fx))


def test_tile_encoder_uint16_packs_the_host_streams():
    planes = _rasters()["padded"]
    n, H, W = planes.shape
    for mode in ("fixed", "dynamic"):
        packed, sizes, offs, sat = TileEncoder(huffman=mode, sample="uint16").encode(
            torch.from_numpy(planes.reshape(n, -1).copy()), H, W, ranges=_ranges(planes))
        streams, esat = _named_streams("padded", mode)
        assert sizes.tolist() == [len(s) for s in streams]
        assert packed[:int(sizes.sum())].numpy().tobytes() == b"".join(streams)
        assert sat.dtype == torch.int64 and sat.tolist() == esat.tolist()


# ---------------------------------------------------------------------- files
def test_geotiff_from_uint16_tiles_roundtrip(tmp_path):
    planes = _rasters()["padded"].copy()
    planes[0, 20:30, 250:] = np.nan
    n, H, W = planes.shape
    rg = [(LO, HI), (0.5, 4.25)]
    q, _ = quantise_u16(planes, rg)
    _, _, scale, offset = TileEncoder.quantiser(rg)
    tx, ty = TileEncoder.tiles(H, W)
    per = tx * ty
    for mode in ("fixed", "dynamic"):
        packed, sizes, offs, _ = TileEncoder(huffman=mode, sample="uint16").encode(
            torch.from_numpy(planes.reshape(n, -1)), H, W, ranges=rg)
        for p in range(n):
            fn = tmp_path / f"{mode}{p}.tif"
            sl = slice(p * per, (p + 1) * per)
            write_tiff_tiles(fn, H, W, packed, offs[sl].tolist(), sizes[sl].tolist(), [0, 10, 0, 0, 0, -10],
                             "EPSG:32630", dtype="uint16", scale=scale[p], offset=offset[p])
            arr, _ = read_tiff(fn)
            assert arr.dtype == np.uint16 and np.array_equal(arr, q[p])
            arr_py, info_py = _read_tiff_py(fn)
            assert np.array_equal(arr_py, q[p])
            info = tiff_info(fn)
            assert info["dtype"] == np.uint16 and info["predictor"] == 2 and info["nodata"] == "65535"
            assert info["scale"] == scale[p] and info["offset"] == offset[p]          # exact: repr round-trips
            assert info_py["scale"] == scale[p] and info_py["offset"] == offset[p] and info_py["nodata"] == "65535"
            val, _ = read_tiff_scaled(fn)
            assert val.dtype == np.float32 and np.array_equal(np.isnan(val), q[p] == 65535)
            ok = q[p] != 65535
            assert np.array_equal(val[ok], (offset[p] + scale[p] * q[p][ok].astype(np.float64)).astype(np.float32))
    assert np.isnan(read_tiff_scaled(tmp_path / "fixed0.tif")[0][20:30, 250:]).all()
    with pytest.raises(ValueError):
        write_tiff_tiles(tmp_path / "x.tif", H, W, packed, [0] * per, [0] * per, scale=1.0)   # float32 takes none


def test_write_tiff_scale_offset_both_writers(tmp_path):
    q = (np.arange(40 * 30, dtype=np.uint16) * 50).reshape(40, 30)
    q[3, 4] = 65535
    sc, of = 0.1 / 3.0, -1e-3 / 7.0
    write_tiff(tmp_path / "n.tif", q, predictor=2, nodata=65535, scale=sc, offset=of)
    _write_tiff_py(tmp_path / "p.tif", q, nodata=65535, scale=sc, offset=of)
    for fn in ("n.tif", "p.tif"):
        for info in (tiff_info(tmp_path / fn), _read_tiff_py(tmp_path / fn)[1]):
            assert info["scale"] == sc and info["offset"] == of and info["nodata"] == "65535"
        val, _ = read_tiff_scaled(tmp_path / fn)
        assert np.isnan(val[3, 4]) and np.isnan(val).sum() == 1
    write_tiff(tmp_path / "f.tif", np.zeros((4, 4), np.float32))
    assert tiff_info(tmp_path / "f.tif")["scale"] is None and tiff_info(tmp_path / "f.tif")["offset"] is None
    assert _read_tiff_py(tmp_path / "f.tif")[1]["scale"] is None


# ---------------------------------------------------------------- KafkaOutput
PARAMS = ["lai", "sm"]
RANGES = {"lai": (0.0, 8.0), "sm": (-0.5, 1.5)}
UNC = {"lai": (0.0, 4.0), "sm": (0.0, 1.0)}


def _dump(out, seed=0):
    """One timestep through the reference-signature writer (CPU planes)."""
    import datetime as dt
    rng = np.random.default_rng(seed)
    mask = np.ones((20, 15), bool)
    mask[::7] = False
    npx = int(mask.sum())
    x = rng.uniform(-1.0, 9.0, 2 * npx)
    x[5] = np.nan
    pinv = np.diag(rng.uniform(0.05, 50.0, 2 * npx))
    ts = dt.datetime(2017, 3, 1)
    out.dump_data(ts, x, None, pinv, mask, 2)
    out.flush()
    mean = np.zeros((2,) + mask.shape, np.float32)
    unc = np.zeros_like(mean)
    for ii in range(2):
        mean[ii][mask] = x[ii::2]
        unc[ii][mask] = 1.0 / np.sqrt(np.diag(pinv)[ii::2])
    return ts, mean, unc


def test_kafka_output_uint16_host_files(tmp_path):
    out = k.KafkaOutput(PARAMS, [0, 10, 0, 0, 0, -10], "EPSG:32630", str(tmp_path), asynchronous=False,
                        sample_type="uint16", encoder="host", ranges=RANGES, unc_ranges=UNC)
    ts, mean, unc = _dump(out)
    total = 0
    for planes, rgs, suffix in ((mean, RANGES, ""), (unc, UNC, "_unc")):
        rg = [rgs[p] for p in PARAMS]
        q, sat = quantise_u16(planes, rg)
        _, _, scale, offset = TileEncoder.quantiser(rg)
        total += int(sat.sum())
        for ii, p in enumerate(PARAMS):
            fn = tmp_path / f"{p}_{ts.strftime('A%Y%j')}{suffix}.tif"
            arr, _ = read_tiff(fn)
            assert arr.dtype == np.uint16 and np.array_equal(arr, q[ii])
            info = tiff_info(fn)
            assert info["predictor"] == 2 and info["nodata"] == "65535"
            assert info["scale"] == scale[ii] and info["offset"] == offset[ii]
    st = out.writer_stats()
    assert st["sample_type"] == "uint16" and st["raster_bytes"] == 4 * 20 * 15 * 2
    assert total > 0 and st["saturated"]["total"] == total and sum(st["saturated"]["last"].values()) == total
    assert "uint16" in st["deflate_backend"]
    assert (read_tiff(tmp_path / f"sm_{ts.strftime('A%Y%j')}.tif")[0] == 65535).sum() == 1       # the NaN


def test_kafka_output_uint16_needs_every_range(tmp_path):
    args = (PARAMS, [0, 10, 0, 0, 0, -10], "EPSG:32630", str(tmp_path))
    with pytest.raises(ValueError, match="sm"):
        k.KafkaOutput(*args, sample_type="uint16", ranges={"lai": (0, 8)}, unc_ranges=UNC)
    with pytest.raises(ValueError, match="unc_ranges"):
        k.KafkaOutput(*args, sample_type="uint16", ranges=RANGES)
    with pytest.raises(ValueError):
        k.KafkaOutput(*args, sample_type="uint16", ranges={"lai": (8, 0), "sm": (0, 1)}, unc_ranges=UNC)
    with pytest.raises(ValueError):
        k.KafkaOutput(*args, ranges=RANGES)                       # float32 takes none
    with pytest.raises(ValueError):
        k.KafkaOutput(*args, sample_type="int16")


def test_kafka_output_default_files_unchanged(tmp_path):
    """With nothing set the float32 files are byte-identical to those of a
    writer built without the new keywords."""
    files = {}
    for name, kw in (("old", {}), ("new", dict(sample_type="float32", ranges=None, unc_ranges=None))):
        out = k.KafkaOutput(PARAMS, [0, 10, 0, 0, 0, -10], "EPSG:32630", str(tmp_path / name), asynchronous=False,
                            predictor=3, strategy="rle", **kw)
        _dump(out)
        st = out.writer_stats()
        assert st["sample_type"] == "float32" and st["raster_bytes"] == 4 * 20 * 15 * 4
        files[name] = {fn.name: fn.read_bytes() for fn in sorted((tmp_path / name).iterdir())}
    assert len(files["old"]) == 4 and files["old"] == files["new"]
    arr, info = read_tiff(tmp_path / "new" / sorted(files["new"])[0])
    assert arr.dtype == np.float32 and info["scale"] is None


# ------------------------------------------------------------------------ CLI
def test_cli_run_with_uint16_output(tmp_path, capsys):
    from kafka_inferenceengine_amd.cli import main
    out = tmp_path / "out"
    argv = ["run", "--sensor", "identity", "--size", "40", "36", "--steps", "2", "--device", "cpu", "--out", str(out),
            "--out-sample", "uint16"]
    for p in k.TIP_PARAMETERS:
        argv += ["--out-range", p, "-1", "7", "--out-unc-range", p, "0", "6"]
    main(argv)
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rec["timesteps"] == 2 and rec["output"]["sample_type"] == "uint16"
    assert rec["output"]["raster_bytes"] == 2 * 14 * 40 * 36 * 2
    assert rec["output"]["saturated"]["total"] == 0
    files = sorted(out.iterdir())
    assert len(files) == 28
    for fn in files:
        info = tiff_info(fn)
        assert info["dtype"] == np.uint16 and info["predictor"] == 2 and info["nodata"] == "65535"
        unc = fn.name.endswith("_unc.tif")
        assert info["offset"] == (0.0 if unc else -1.0) and info["scale"] == (6.0 if unc else 8.0) / 65534.0
        val, _ = read_tiff_scaled(fn)
        assert np.isfinite(val).all() and val.min() >= info["offset"] and val.max() <= info["offset"] + 65534 * info["scale"]
    with pytest.raises(ValueError, match=k.TIP_PARAMETERS[-1]):
        main(argv[:-4])                                           # one uncertainty range missing
