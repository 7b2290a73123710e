// sanitize_inflate.cpp — AddressSanitizer / UBSan driver for the GeoTIFF tile
// decoder's shared source (csrc/kf_inflate.h) through the host runner.
//
// host_inflate_tiles runs over a valid corpus (stored, fixed and dynamic
// streams of zlib at several levels and strategies, a multi-block stream with
// an empty stored block, distance 32768, 15-bit codes, and the project's own
// encoder's fixed and dynamic float32 streams with predictor 3) and over the
// malformed set of one small dynamic stream (truncated at every byte, each of
// its first 400 bits flipped, a corrupt NLEN, a corrupt Adler-32, the raw size
// one byte too small and too large), every stream in an exactly-sized input
// allocation of its own and every destination exactly sized.  A valid stream
// must give zlib's bytes; a malformed one a status and a zeroed tile, unless
// zlib itself decodes it to the right bytes.  A clean exit is the memory-safety
// evidence for the shared source.  Built and run by tests/test_sanitize_inflate.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer
//       -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Icsrc -fopenmp
//       tests/native/sanitize_inflate.cpp csrc/kf_host.cpp -lz
#include <zlib.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "kf_deflate.h"
#include "kf_inflate.h"
#include "kf_launch.h"

using namespace kf;

namespace {

int failures = 0;
void check(bool ok, const char* what) {
  if (!ok) {
    std::fprintf(stderr, "FAIL: %s\n", what);
    ++failures;
  }
}

using Bytes = std::vector<uint8_t>;
constexpr int T = DFL_TILE;
constexpr int64_t RAW16 = (int64_t)T * T * 2;

Bytes deflate_with(const Bytes& raw, int level, int strategy, size_t flush_at = 0) {
  z_stream zs{};
  check(deflateInit2(&zs, level, Z_DEFLATED, 15, 8, strategy) == Z_OK, "deflateInit2");
  Bytes out(deflateBound(&zs, (uLong)raw.size()) + 64);
  zs.next_out = out.data();
  zs.avail_out = (uInt)out.size();
  zs.next_in = const_cast<Bytef*>(raw.data());
  if (flush_at) {
    zs.avail_in = (uInt)flush_at;
    check(deflate(&zs, Z_FULL_FLUSH) == Z_OK, "deflate flush");
  }
  zs.avail_in = (uInt)(raw.size() - flush_at);
  check(deflate(&zs, Z_FINISH) == Z_STREAM_END, "deflate finish");
  out.resize(zs.total_out);
  deflateEnd(&zs);
  return out;
}

// One tile through the host runner: the stream in an allocation of exactly its
// size, the destination exactly one tile.  Returns the status.
int32_t decode(const Bytes& stream, int elem, int pred, int64_t raw_bytes, Bytes& tile) {
  std::unique_ptr<uint8_t[]> in(new uint8_t[stream.size()]);      // exactly sized (size 0 too)
  if (!stream.empty()) std::memcpy(in.get(), stream.data(), stream.size());
  const int64_t off = 0, size = (int64_t)stream.size();
  const int32_t rc[2] = {0, 0};
  int32_t status = -1;
  tile.assign((size_t)T * T * elem, 0xAA);
  InfArgs a{};
  a.comp = in.get();
  a.comp_bytes = size;
  a.offs = &off;
  a.sizes = &size;
  a.tile_rc = rc;
  a.ntiles = 1;
  a.tile = T;
  a.elem_bytes = elem;
  a.predictor = pred;
  a.raw_bytes = raw_bytes;
  a.r0 = 0;
  a.r1 = T;
  a.c0 = 0;
  a.c1 = T;
  a.dst = tile.data();
  a.ld = T;
  a.status = &status;
  check(host_inflate_tiles(a) == 0, "host_inflate_tiles accepts the arguments");
  return status;
}

bool all_zero(const Bytes& b) {
  for (uint8_t v : b)
    if (v) return false;
  return true;
}

bool zlib_gives(const Bytes& stream, const Bytes& raw) {
  Bytes out(raw.size() + 1);
  uLongf n = (uLongf)out.size();
  return uncompress(out.data(), &n, stream.data(), (uLong)stream.size()) == Z_OK && n == raw.size() &&
         std::memcmp(out.data(), raw.data(), raw.size()) == 0;
}

void valid(const char* name, const Bytes& stream, const Bytes& raw) {
  Bytes tile;
  check(decode(stream, 2, 1, RAW16, tile) == INF_OK, name);
  check(tile == raw, name);
}

}  // namespace

int main() {
  std::mt19937 rng(5);
  std::vector<Bytes> raws;
  {
    Bytes smooth((size_t)RAW16), random((size_t)RAW16), zeros((size_t)RAW16, 0), repeat, geo((size_t)RAW16);
    std::normal_distribution<float> nd(0.f, 12.f);
    for (int y = 0; y < T; ++y)
      for (int x = 0; x < T; ++x) {
        const uint16_t v = (uint16_t)(3000.f + 1500.f * std::sin(x / 31.f) * std::cos(y / 19.f) + nd(rng));
        std::memcpy(&smooth[((size_t)y * T + x) * 2], &v, 2);
      }
    for (auto& b : random) b = (uint8_t)rng();
    Bytes block(32768);
    for (auto& b : block) b = (uint8_t)rng();
    for (int k = 0; k < 4; ++k) repeat.insert(repeat.end(), block.begin(), block.end());
    std::geometric_distribution<int> gd(0.5);
    for (auto& b : geo) b = (uint8_t)std::min(gd(rng), 255);
    raws = {smooth, random, zeros, repeat, geo};
  }
  bool seen[3] = {false, false, false};
  int nvalid = 0;
  for (const Bytes& raw : raws) {
    std::vector<Bytes> streams;
    for (int lv : {0, 1, 6, 9}) streams.push_back(deflate_with(raw, lv, Z_DEFAULT_STRATEGY));
    for (int st : {Z_FIXED, Z_RLE, Z_HUFFMAN_ONLY}) streams.push_back(deflate_with(raw, 6, st));
    streams.push_back(deflate_with(raw, 6, Z_DEFAULT_STRATEGY, 50000));
    for (const Bytes& s : streams) {
      seen[(s[2] >> 1) & 3] = true;
      valid("zlib stream decodes to the raw tile", s, raw);
      ++nvalid;
    }
  }
  check(seen[0] && seen[1] && seen[2], "stored, fixed and dynamic first blocks in the corpus");

  // the project's own encoder: float32 tiles, predictor 3, fixed and dynamic blocks
  {
    const int H = 300, W = 520;
    std::vector<float> src((size_t)H * W);
    std::normal_distribution<float> nd(0.f, 1.f);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        float f = std::sin(x / 17.f) * std::cos(y / 23.f) + 0.01f * nd(rng);
        if ((y / 40 + x / 40) % 5 == 0) f = 0.f;
        src[(size_t)y * W + x] = f;
      }
    for (int mode : {DFL_MODE_FIXED, DFL_MODE_DYNAMIC}) {
      DflArgs e{};
      e.src = src.data();
      e.plane_ld = (int64_t)H * W;
      e.H = H;
      e.W = W;
      e.nplanes = 1;
      e.tiles_x = (W + T - 1) / T;
      e.tiles_y = (H + T - 1) / T;
      e.mode = mode;
      const int nt = e.tiles_x * e.tiles_y;
      Bytes enc((size_t)nt * DFL_BOUND);
      std::vector<uint32_t> sizes((size_t)nt);
      e.out = enc.data();
      e.sizes = sizes.data();
      check(host_deflate_tiles(e) == 0, "host_deflate_tiles");
      // all tiles in one call, packed back to back in an exactly-sized buffer, into the exactly-sized raster
      std::vector<int64_t> offs((size_t)nt), szs((size_t)nt);
      std::vector<int32_t> rc;
      int64_t total = 0;
      for (int t = 0; t < nt; ++t) {
        offs[t] = total;
        szs[t] = sizes[t];
        total += sizes[t];
        rc.push_back(t / e.tiles_x);
        rc.push_back(t % e.tiles_x);
      }
      std::unique_ptr<uint8_t[]> packed(new uint8_t[(size_t)total]);
      for (int t = 0; t < nt; ++t) std::memcpy(packed.get() + offs[t], enc.data() + (size_t)t * DFL_BOUND, sizes[t]);
      std::vector<float> out((size_t)H * W, -1.f);
      std::vector<int32_t> status((size_t)nt, -1);
      InfArgs a{};
      a.comp = packed.get();
      a.comp_bytes = total;
      a.offs = offs.data();
      a.sizes = szs.data();
      a.tile_rc = rc.data();
      a.ntiles = nt;
      a.tile = T;
      a.elem_bytes = 4;
      a.predictor = 3;
      a.raw_bytes = DFL_RAW;
      a.r0 = 0;
      a.r1 = H;
      a.c0 = 0;
      a.c1 = W;
      a.dst = out.data();
      a.ld = W;
      a.status = status.data();
      check(host_inflate_tiles(a) == 0, "host_inflate_tiles (float32, predictor 3)");
      for (int s : status) check(s == INF_OK, "own encoder stream decodes");
      check(std::memcmp(out.data(), src.data(), src.size() * 4) == 0, "encode -> decode gives the input's bits");
      nvalid += nt;
    }
  }

  // the malformed set of one small dynamic stream
  Bytes tile = raws[0];
  for (int y = 4; y < T; ++y) std::memcpy(&tile[(size_t)y * T * 2], &tile[(size_t)(y % 4) * T * 2], (size_t)T * 2);
  const Bytes s = deflate_with(tile, 9, Z_DEFAULT_STRATEGY);
  check(((s[2] >> 1) & 3) == 2, "the small stream starts with a dynamic block");
  valid("the small dynamic stream", s, tile);
  int nbad = 0, nsame = 0;
  Bytes got;
  auto malformed = [&](const Bytes& stream, int64_t raw_bytes, const Bytes& want, const char* what) {
    const int32_t st = decode(stream, 2, 1, raw_bytes, got);
    if (raw_bytes == RAW16 && zlib_gives(stream, want)) {
      check(st == INF_OK && got == want, "a damaged stream zlib still decodes: the same bytes");
      ++nsame;
      return;
    }
    check(st != INF_OK && st > 0 && st < INF_NSTATUS, what);
    check(all_zero(got), "a failed tile is zeroed");
    ++nbad;
  };
  for (size_t k = 0; k < s.size(); ++k) malformed(Bytes(s.begin(), s.begin() + k), RAW16, tile, "truncated stream");
  for (int bit = 0; bit < 400; ++bit) {
    Bytes b = s;
    b[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
    malformed(b, RAW16, tile, "flipped bit");
  }
  {
    Bytes st = deflate_with(raws[1], 0, Z_DEFAULT_STRATEGY);
    st[5] ^= 0x10;
    malformed(st, RAW16, raws[1], "corrupt NLEN");
    Bytes b = s;
    b.back() ^= 1;
    malformed(b, RAW16, tile, "corrupt Adler-32");
    malformed(s, RAW16 - 1, tile, "raw size one byte too small");
    malformed(s, RAW16 + 1, tile, "raw size one byte too large");
  }
  std::printf("%d valid tiles, %d malformed streams with a status, %d zlib also decodes\n", nvalid, nbad, nsame);
  if (failures) {
    std::fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  std::printf("sanitize_inflate ok\n");
  return 0;
}
