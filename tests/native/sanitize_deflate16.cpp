// sanitize_deflate16.cpp — AddressSanitizer / UBSan driver for the 16-bit sample
// format of the GeoTIFF tile encoder (csrc/kf_deflate.h: dfl_quantise,
// DFL_FMT_U16) through the host runner.
//
// host_deflate_tiles runs in the fixed and the dynamic-Huffman mode, with
// exactly-sized buffers, on a smooth field, a constant tile (rows shorter than a
// word), full-range noise, the adversarial tile (alternating 0 / 65534 columns:
// wrap-around differences; rows that start with 258, 259, 260 and 512 equal
// bytes), a tile with a NaN block and out-of-range values, and the padded
// shapes 300 x 260 (2 planes) and 1 x 1.  Every stream must inflate (zlib
// checks the Adler-32) to exactly the predictor-2 bytes of the tile quantised
// by host_quantise_u16, a dynamic stream is never larger than the fixed one,
// the dynamic path with the choice forced to the fixed block gives the fixed
// mode's bytes, and the saturation counters of the encoder and the quantiser
// agree.  Built and run by tests/test_sanitize_deflate16.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer
//       -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Icsrc -fopenmp
//       tests/native/sanitize_deflate16.cpp csrc/kf_host.cpp -lz
#include <zlib.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
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

const double LO = -0.37, HI = 6.2;
const float QA = (float)(65534.0 / (HI - LO)), QB = (float)(-LO * 65534.0 / (HI - LO));

struct Streams {
  std::vector<std::vector<uint8_t>> tiles;
  std::vector<uint32_t> sat;
  int rc;
};

Streams encode(const std::vector<float>& src, int H, int W, int nplanes, int mode) {
  const std::vector<float> qa((size_t)nplanes, QA), qb((size_t)nplanes, QB);
  DflArgs a{};
  a.src = src.data();
  a.plane_ld = (int64_t)H * W;
  a.H = H;
  a.W = W;
  a.nplanes = nplanes;
  a.tiles_x = (W + DFL_TILE - 1) / DFL_TILE;
  a.tiles_y = (H + DFL_TILE - 1) / DFL_TILE;
  a.mode = mode;
  a.fmt = DFL_FMT_U16;
  a.qa = qa.data();
  a.qb = qb.data();
  const int nt = nplanes * a.tiles_x * a.tiles_y;
  std::vector<uint8_t> out((size_t)nt * DFL_BOUND16);
  std::vector<uint32_t> sizes((size_t)nt);
  Streams s;
  s.sat.assign((size_t)nplanes, 0u);
  a.out = out.data();
  a.sizes = sizes.data();
  a.scratch = nullptr;
  a.sat = s.sat.data();
  s.rc = host_deflate_tiles(a);
  for (int t = 0; t < nt; ++t)
    s.tiles.emplace_back(out.begin() + (size_t)t * DFL_BOUND16, out.begin() + (size_t)t * DFL_BOUND16 + sizes[t]);
  return s;
}

void run(const char* name, const std::vector<float>& src, int H, int W, int nplanes) {
  const Streams fx = encode(src, H, W, nplanes, DFL_MODE_FIXED);
  const Streams dy = encode(src, H, W, nplanes, DFL_MODE_DYNAMIC);
  const Streams ff = encode(src, H, W, nplanes, DFL_MODE_DYNAMIC_FORCE_FIXED);
  check(fx.rc == 0 && dy.rc == 0 && ff.rc == 0, name);
  const std::vector<float> qa((size_t)nplanes, QA), qb((size_t)nplanes, QB);
  std::vector<uint16_t> q((size_t)nplanes * H * W);
  std::vector<uint32_t> sat((size_t)nplanes, 0u);
  check(host_quantise_u16(src.data(), (int64_t)H * W, (int64_t)H * W, nplanes, qa.data(), qb.data(), q.data(),
                          sat.data()) == 0, "quantiser runs");
  check(fx.sat == sat && dy.sat == sat && ff.sat == sat, "saturation counters agree");
  const int tx = (W + DFL_TILE - 1) / DFL_TILE, ty = (H + DFL_TILE - 1) / DFL_TILE;
  std::vector<uint8_t> raw((size_t)DFL_RAW16), ref((size_t)DFL_RAW16);
  for (size_t t = 0; t < fx.tiles.size(); ++t) {
    const int p = (int)t / (tx * ty), tt = (int)t % (tx * ty), y0 = tt / tx * DFL_TILE, x0 = tt % tx * DFL_TILE;
    for (int r = 0; r < DFL_TILE; ++r) {
      uint16_t prev = 0;
      for (int c = 0; c < DFL_TILE; ++c) {
        const bool in = y0 + r < H && x0 + c < W;
        const uint16_t v = in ? q[((size_t)p * H + y0 + r) * W + x0 + c] : (uint16_t)0;
        const uint16_t d = (uint16_t)(v - prev);
        prev = v;
        ref[((size_t)r * DFL_TILE + c) * 2] = (uint8_t)(d & 0xFFu);
        ref[((size_t)r * DFL_TILE + c) * 2 + 1] = (uint8_t)(d >> 8);
      }
    }
    for (const Streams* s : {&fx, &dy}) {
      uLongf n = (uLongf)raw.size();
      const int z = uncompress(raw.data(), &n, s->tiles[t].data(), (uLong)s->tiles[t].size());
      check(z == Z_OK && n == (uLongf)DFL_RAW16, "stream inflates to one tile");
      check(raw == ref, "the tile's predictor-2 bytes");
    }
    check(dy.tiles[t].size() <= fx.tiles[t].size(), "dynamic tile no larger than fixed");
    check(ff.tiles[t] == fx.tiles[t], "forced fixed block equals the fixed mode");
  }
  std::printf("%s: %zu tiles ok\n", name, fx.tiles.size());
}

float value_of(uint32_t q) { return (float)(LO + (HI - LO) / 65534.0 * (double)q); }

}  // namespace

int main() {
  const int T = DFL_TILE;
  std::mt19937 rng(7);
  std::normal_distribution<float> nd(0.f, 1.f);
  std::uniform_real_distribution<float> ud((float)LO, (float)HI);

  std::vector<float> smooth((size_t)T * T);
  for (int y = 0; y < T; ++y)
    for (int x = 0; x < T; ++x) smooth[(size_t)y * T + x] = 2.9f + 2.5f * std::sin(x / 37.f) * std::cos(y / 23.f) + 0.02f * nd(rng);
  run("smooth", smooth, T, T, 1);

  std::vector<float> cst((size_t)T * T, 1.25f);
  run("const", cst, T, T, 1);

  std::vector<float> noise((size_t)T * T);
  for (auto& v : noise) v = ud(rng);
  run("noise", noise, T, T, 1);

  std::vector<float> adv((size_t)T * T);
  for (int y = 0; y < T; ++y)
    for (int x = 0; x < T; ++x) adv[(size_t)y * T + x] = value_of((x & 1) ? 65534u : 0u);
  const int runs[4] = {258, 259, 260, 512};
  for (int k = 0; k < 4; ++k) {
    uint8_t b[512];
    for (int i = 0; i < 512; ++i) {
      const int j = i - runs[k];
      b[i] = j < 0 ? 2 : j == 0 ? 6 : (j % 2 == 0) ? (uint8_t)(4 + 2 * (j / 2 % 50)) : 0;
    }
    uint16_t q = 0;
    for (int c = 0; c < T; ++c) {
      q = (uint16_t)(q + (uint16_t)(b[2 * c] | (b[2 * c + 1] << 8)));
      check(q != 65535, "adversarial samples stay below nodata");
      adv[(size_t)(10 + k) * T + c] = value_of(q);
    }
  }
  run("adv", adv, T, T, 1);

  std::vector<float> nan = smooth;
  for (int y = 40; y < 90; ++y)
    for (int x = 100; x < 180; ++x) nan[(size_t)y * T + x] = std::numeric_limits<float>::quiet_NaN();
  for (int x = 0; x < T; ++x) nan[(size_t)7 * T + x] = (x & 1) ? 1e30f : -std::numeric_limits<float>::infinity();
  run("nan", nan, T, T, 1);

  const int H = 300, W = 260;
  std::vector<float> pad((size_t)2 * H * W);
  for (int p = 0; p < 2; ++p)
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        float f = 2.9f + 2.5f * std::sin(x / (17.f + p)) * std::cos(y / 23.f) + 0.02f * nd(rng);
        if ((y / 40 + x / 40) % 5 == 0) f = 0.f;
        pad[((size_t)p * H + y) * W + x] = f;
      }
  run("padded", pad, H, W, 2);

  std::vector<float> one(1, 3.f);
  run("one", one, 1, 1, 1);

  if (failures) {
    std::fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  std::printf("sanitize_deflate16 ok\n");
  return 0;
}
