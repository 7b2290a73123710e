"""Shared inputs of the tile-decoder tests (tests/test_inflate.py on the host
runner, tests/test_gpu_inflate.py on the device): a corpus of 256 x 256 tiles
compressed every way zlib offers, the project's own encoder streams, and the
malformed variants of one small dynamic stream.  Built at run time from seeded
numpy; the oracle is zlib / numpy."""
import functools
import zlib

import numpy as np
import torch

from kafka_inferenceengine_amd.ops.kernels import TileDecoder, TileEncoder, ext

T = 256
RAW16 = T * T * 2


def btype(stream: bytes) -> int:
    """BTYPE of a zlib stream's first block (bits 1-2 behind the 2-byte header)."""
    return (stream[2] >> 1) & 3


@functools.lru_cache(maxsize=None)
def raw_tiles():
    """name -> 131,072 raw bytes of a 256 x 256 uint16 tile."""
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:T, 0:T]
    smooth = (3000 + 1500 * np.sin(xx / 31.0) * np.cos(yy / 19.0) + rng.normal(0, 12, (T, T))).astype(np.uint16)
    block = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    geo = np.minimum(rng.geometric(0.5, RAW16) - 1, 255).astype(np.uint8)     # P(v) ~ 2^-(v+1): 15-bit codes
    return {"smooth": smooth.tobytes(), "random": rng.integers(0, 256, RAW16, dtype=np.uint8).tobytes(),
            "zeros": bytes(RAW16), "repeat": block * 4, "geometric": geo.tobytes()}


def _compress(raw, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    return c.compress(raw) + c.flush()


@functools.lru_cache(maxsize=None)
def corpus16():
    """[(name, stream, raw)] of the uint16 tiles: levels 0 / 1 / 6 / 9, the
    strategies Z_FIXED / Z_RLE / Z_HUFFMAN_ONLY, and a stream with a
    Z_FULL_FLUSH in the middle (several blocks, an empty stored block)."""
    out = []
    for name, raw in raw_tiles().items():
        for lv in (0, 1, 6, 9):
            out.append((f"{name}-l{lv}", _compress(raw, lv), raw))
        for sname, st in (("fixed", zlib.Z_FIXED), ("rle", zlib.Z_RLE), ("huff", zlib.Z_HUFFMAN_ONLY)):
            out.append((f"{name}-{sname}", _compress(raw, 6, st), raw))
        c = zlib.compressobj(6)
        out.append((f"{name}-flush", c.compress(raw[:50000]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(raw[50000:])
                    + c.flush(), raw))
    return out


@functools.lru_cache(maxsize=None)
def float_planes():
    """The 300 x 520 x 2 float32 raster of the encode -> decode round trip."""
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:300, 0:520]
    out = []
    for i in range(2):
        f = np.sin(xx / (17.0 + i)) * np.cos(yy / 23.0) + 0.01 * rng.standard_normal((300, 520))
        f[(yy // 40 + xx // 40) % 5 == 0] = 0.0
        out.append((f * (i + 1)).astype(np.float32))
    return np.stack(out)


def encoder_streams(huffman, device="cpu"):
    """The project's own streams of float_planes(): (packed uint8 tensor, sizes, offsets, tile_rc int32 [n, 2])
    on ``device``; tiles plane-major, row-major within a plane."""
    planes = torch.from_numpy(float_planes()).reshape(2, -1).to(device)
    packed, sizes, offs = TileEncoder(huffman).encode(planes, 300, 520)
    tx, ty = TileEncoder.tiles(300, 520)
    rc = torch.tensor([[r, c] for _ in range(2) for r in range(ty) for c in range(tx)], dtype=torch.int32)
    return packed, sizes, offs, rc.to(device)


def pack(streams, device="cpu"):
    """-> (data uint8, offsets int64, sizes int64) of byte strings back to back."""
    sizes = np.array([len(s) for s in streams], np.int64)
    offs = np.cumsum(sizes) - sizes
    data = np.frombuffer(b"".join(streams), np.uint8).copy()
    return (torch.from_numpy(data).to(device), torch.from_numpy(offs).to(device), torch.from_numpy(sizes).to(device))


def decode_raw(streams, device="cpu", elem_bytes=2, raw_bytes=None, decoder=None):
    """Every stream as one tile, stacked vertically, predictor 1: -> (bytes [n, tile bytes] uint8 numpy,
    status numpy).  The destination is what the decoder wrote: the raw tile, or zeros."""
    n = len(streams)
    data, offs, sizes = pack(streams, device)
    rc = torch.tensor([[i, 0] for i in range(n)], dtype=torch.int32, device=device)
    dt = torch.int16 if elem_bytes == 2 else torch.float32
    out = torch.full((n * T, T), 21845 if elem_bytes == 2 else 7.0, dtype=dt, device=device)
    _, st = (decoder or TileDecoder()).decode(data, offs, sizes, rc, tile=T, elem_bytes=elem_bytes, predictor=1,
                                             window=(0, n * T, 0, T), out=out, raw_bytes=raw_bytes)
    return out.cpu().numpy().view(np.uint8).reshape(n, -1), st.cpu().numpy()


# ---------------------------------------------------------------- malformed
@functools.lru_cache(maxsize=None)
def small_dynamic():
    """One small valid dynamic-Huffman stream and its raw tile."""
    raw = raw_tiles()["smooth"]
    rows = np.frombuffer(raw, np.uint16).reshape(T, T)
    tile = np.tile(rows[:4], (T // 4, 1)).tobytes()        # 4 distinct rows: a short stream with long matches
    s = _compress(tile, 9)
    assert btype(s) == 2
    return s, tile


def stored_stream():
    raw = raw_tiles()["random"]
    return _compress(raw, 0), raw


def zlib_verdict(stream, raw):
    """True when zlib decodes ``stream`` to exactly ``raw``."""
    try:
        return zlib.decompress(stream) == raw
    except zlib.error:
        return False


@functools.lru_cache(maxsize=None)
def malformed():
    """[(name, stream, raw size, raw the stream is meant to give)]: the
    truncations at every byte, the first 400 single-bit flips, a corrupt NLEN,
    a corrupt Adler-32, and the raw size one byte too small / too large."""
    s, tile = small_dynamic()
    out = [(f"trunc{k}", s[:k], RAW16, tile) for k in range(len(s))]
    for bit in range(400):
        b = bytearray(s)
        b[bit >> 3] ^= 1 << (bit & 7)
        out.append((f"flip{bit}", bytes(b), RAW16, tile))
    st, sraw = stored_stream()
    b = bytearray(st)
    b[5] ^= 0x10                                            # 78 01 | 00 | LEN LEN | NLEN NLEN
    out.append(("nlen", bytes(b), RAW16, sraw))
    b = bytearray(s)
    b[-1] ^= 1
    out.append(("adler", bytes(b), RAW16, tile))
    out.append(("raw-1", s, RAW16 - 1, tile))
    out.append(("raw+1", s, RAW16 + 1, tile))
    return out


GPU_MALFORMED = ("trunc0", "trunc1", "trunc2", "trunc40", "flip0", "flip17", "flip18", "flip40", "flip200",
                 "flip399", "nlen", "adler")


def status_names():
    return list(ext().INF_STATUS_NAMES)
