// sanitize_deflate.cpp — AddressSanitizer / UBSan driver for the GeoTIFF tile
// encoder's shared source (csrc/kf_deflate.h) through the host runner.
//
// host_deflate_tiles runs in the fixed and the dynamic-Huffman mode on a
// constant tile (rows shorter than a word), the adversarial tile (one noise
// row in a two-valued tile: 11..15-bit literals) and a padded (300, 520)
// raster, with exactly-sized buffers.  Every stream must inflate (zlib checks
// the Adler-32) to 262144 bytes, a dynamic stream is never larger than the
// fixed one, and the dynamic path with the choice forced to the fixed block
// gives the fixed mode's bytes.  The size function is also checked on a
// histogram where the fixed block wins.  This covers the shared header, not
// the device-only row scratch.  Built and run by tests/test_sanitize_deflate.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer
//       -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Icsrc -fopenmp
//       tests/native/sanitize_deflate.cpp csrc/kf_host.cpp -lz
#include <zlib.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "kf_deflate.h"
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

struct Streams {
  std::vector<std::vector<uint8_t>> tiles;
  int rc;
};

Streams encode(const std::vector<float>& src, int H, int W, int nplanes, int mode) {
  DflArgs a{};
  a.src = src.data();
  a.plane_ld = (int64_t)H * W;
  a.H = H;
  a.W = W;
  a.nplanes = nplanes;
  a.tiles_x = (W + DFL_TILE - 1) / DFL_TILE;
  a.tiles_y = (H + DFL_TILE - 1) / DFL_TILE;
  a.mode = mode;
  const int nt = nplanes * a.tiles_x * a.tiles_y;
  std::vector<uint8_t> out((size_t)nt * DFL_BOUND);
  std::vector<uint32_t> sizes((size_t)nt);
  a.out = out.data();
  a.sizes = sizes.data();
  a.scratch = nullptr;
  Streams s;
  s.rc = host_deflate_tiles(a);
  for (int t = 0; t < nt; ++t)
    s.tiles.emplace_back(out.begin() + (size_t)t * DFL_BOUND, out.begin() + (size_t)t * DFL_BOUND + sizes[t]);
  return s;
}

void run(const char* name, const std::vector<float>& src, int H, int W, int nplanes, bool expect_dynamic) {
  const Streams fx = encode(src, H, W, nplanes, DFL_MODE_FIXED);
  const Streams dy = encode(src, H, W, nplanes, DFL_MODE_DYNAMIC);
  const Streams ff = encode(src, H, W, nplanes, DFL_MODE_DYNAMIC_FORCE_FIXED);
  check(fx.rc == 0 && dy.rc == 0 && ff.rc == 0, name);
  std::vector<uint8_t> raw((size_t)DFL_RAW);
  for (size_t t = 0; t < fx.tiles.size(); ++t) {
    for (const Streams* s : {&fx, &dy}) {
      uLongf n = (uLongf)raw.size();
      const int z = uncompress(raw.data(), &n, s->tiles[t].data(), (uLong)s->tiles[t].size());
      check(z == Z_OK && n == (uLongf)DFL_RAW, "stream inflates to one tile");
    }
    check(dy.tiles[t].size() <= fx.tiles[t].size(), "dynamic tile no larger than fixed");
    check(ff.tiles[t] == fx.tiles[t], "forced fixed block equals the fixed mode");
    if (expect_dynamic) check(((dy.tiles[t][2] >> 1) & 3) == 2, "BTYPE 10");
  }
  std::printf("%s: %zu tiles ok\n", name, fx.tiles.size());
}

// a histogram on which the fixed block wins: the choice must fall back, and
// both sizes must be exact
void size_function() {
  uint32_t freq[DFL_NSYM] = {0};
  freq[7] = 1;
  freq[256] = 1;
  DflTable t;
  DflWork k;
  int used = 0;
  for (int s = 0; s < DFL_NSYM; ++s) {
    const int r = dfl_rank(freq, DFL_NSYM, s);
    if (r >= 0) {
      k.sorted[r] = (uint16_t)s;
      ++used;
    }
  }
  check(used == 2, "two used symbols");
  const uint64_t dyn = dfl_dynamic_table(freq, used, t, k);
  check(t.len[7] == 1 && t.len[256] == 1, "two symbols: one bit each");
  check(dfl_fixed_bits(freq) == 3 + 8 + 7, "fixed block bits");
  check(dyn > dfl_fixed_bits(freq), "tiny block: the fixed code wins");
  uint64_t n = 0;
  dfl_write_block_header(t, [&](uint32_t, int len) { n += (uint64_t)len; });
  check(n == t.head_bits && dyn == t.head_bits + 2, "dynamic header bits exact");
  dfl_choose_table(freq, used, false, t, k);
  check(!t.dynamic && t.dist_len == 5 && t.head_bits == 3 && t.block_bits == 18, "fallback to the fixed table");
  for (int v = 0; v < 256; ++v) {
    uint32_t b0, b1;
    int l0, l1;
    dfl_lit((uint32_t)v, b0, l0);
    dfl_table_token(t, (uint32_t)v, 0, b1, l1);
    check(b0 == b1 && l0 == l1, "fixed table literal");
  }
  for (int L = 3; L <= 258; ++L) {
    uint32_t b0, b1;
    int l0, l1;
    dfl_match(L, b0, l0);
    dfl_table_token(t, 0u, L, b1, l1);
    check(b0 == b1 && l0 == l1, "fixed table match");
  }
}

}  // namespace

int main() {
  const int T = DFL_TILE;
  std::mt19937 rng(7);
  std::normal_distribution<float> nd(0.f, 1.f);

  std::vector<float> cst((size_t)T * T, 0.5f);
  run("const", cst, T, T, 1, false);

  std::vector<float> adv((size_t)T * T);
  for (int y = 0; y < T; ++y)
    for (int x = 0; x < T; ++x) adv[(size_t)y * T + x] = y == 100 ? nd(rng) : (x & 1) ? 0.75f : 0.5f;
  run("adv", adv, T, T, 1, true);

  const int H = 300, W = 520;
  std::vector<float> pad((size_t)2 * H * W);
  for (int p = 0; p < 2; ++p)
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        float f = std::sin(x / (17.f + p)) * std::cos(y / 23.f) + 0.01f * nd(rng);
        if ((y / 40 + x / 40) % 5 == 0) f = 0.f;
        pad[((size_t)p * H + y) * W + x] = f * (p + 1);
      }
  run("padded", pad, H, W, 2, false);

  size_function();
  if (failures) {
    std::fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  std::printf("sanitize_deflate ok\n");
  return 0;
}
