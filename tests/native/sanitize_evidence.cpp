// sanitize_evidence.cpp — AddressSanitizer / UBSan driver for the joint
// innovation statistic on the host runner (kf_core.h pixel_innovation<NP, true>,
// shared verbatim with the device kernel).  Every buffer is exactly sized,
// so an out-of-bounds index of the n x n accumulator, delta or the band walk
// faults under -fsanitize=address.  Built and run by tests/test_sanitize_evidence.py:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer
//       -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Icsrc -fopenmp
//       tests/native/sanitize_evidence.cpp csrc/kf_host.cpp
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "kf_launch.h"

using namespace kf;

namespace {

std::mt19937 rng(4321);
float unif(float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); }

int failures = 0;
void check(bool ok, const char* what) {
  if (!ok) {
    std::fprintf(stderr, "FAIL: %s\n", what);
    ++failures;
  }
}

// linear bands on float32 (y, w) pairs, a fifth of the samples without an observation; with and
// without the joint outputs, both kinds, a gate with screened planes; one unscreenable pixel
void run(int np, int nb, int64_t N) {
  const int nt = np * (np + 1) / 2;
  std::vector<float> x((size_t)np * N), P((size_t)nt * N, 0.f);
  for (auto& v : x) v = unif(0.25f, 0.75f);
  for (int64_t p = 0; p < N; ++p)
    for (int i = 0; i < np; ++i)
      for (int j = i; j < np; ++j)
        P[(size_t)tri(np, i, j) * N + p] = (i == j) ? 4.f + unif(0.f, 1.f) : unif(-0.1f, 0.1f);
  if (N > 2) P[(size_t)(nt - 1) * N + 1] = NAN;
  std::vector<std::vector<float>> y(nb, std::vector<float>((size_t)N)), w(nb, std::vector<float>((size_t)N));
  std::vector<std::vector<float>> scr(nb, std::vector<float>((size_t)N));
  std::vector<BandDesc> bands((size_t)nb);
  std::vector<void*> planes((size_t)nb);
  std::vector<int32_t> grp((size_t)nb);
  for (int b = 0; b < nb; ++b) {
    BandDesc& bd = bands[b];
    std::memset(&bd, 0, sizeof(bd));
    bd.op = OP_LINEAR;
    bd.obs = OBS_F32;
    for (int j = 0; j < np; ++j) bd.coef[j] = unif(-0.3f, 0.3f);
    bd.offset = unif(0.05f, 0.2f);
    for (int64_t p = 0; p < N; ++p) {
      y[b][p] = unif(-0.5f, 1.f);
      w[b][p] = unif(0.f, 1.f) < 0.2f ? 0.f : unif(1.f, 400.f);
    }
    bd.y = y[b].data();
    bd.w = w[b].data();
    planes[b] = scr[b].data();
    grp[b] = b % 3;
  }
  std::vector<float> z((size_t)nb * N), chi2((size_t)N), d2((size_t)N), logdet((size_t)N);
  std::vector<uint8_t> nobs((size_t)N), nrej((size_t)N), status((size_t)N);
  for (int kind : {MARG_PRECISION, MARG_COVARIANCE}) {
    InnovationArgs a{};
    a.N = N; a.ld = N; a.ldz = N; a.kind = kind; a.nb = nb; a.scope = INNOV_SCOPE_GROUP; a.gate = 2.f;
    a.x = x.data(); a.p = P.data(); a.bands = bands.data(); a.grp = grp.data();
    a.z = z.data(); a.chi2 = chi2.data(); a.nobs = nobs.data(); a.nrej = nrej.data(); a.status = status.data();
    a.screened = planes.data();
    std::vector<float> chi2_plain;
    check(host_innovation(np, a) == 0, "host_innovation rc");
    chi2_plain = chi2;
    a.d2 = d2.data(); a.logdet = logdet.data();
    check(host_innovation(np, a) == 0, "host_innovation joint rc");
    check(std::memcmp(chi2_plain.data(), chi2.data(), sizeof(float) * (size_t)N) == 0, "chi2 bits unmoved");
    for (int64_t p = 0; p < N; ++p) {
      const bool bad = status[p] != 0;
      check(bad == (N > 2 && p == 1), "only the NaN pixel is unscreenable");
      const bool fin = std::isfinite(d2[p]) && std::isfinite(logdet[p]) && d2[p] >= 0.f;
      check(bad ? std::isnan(d2[p]) && std::isnan(logdet[p]) : fin, "d2 / logdet NaN exactly on the unscreenable pixel");
      if (!bad && nobs[p] == 0) check(d2[p] == 0.f && logdet[p] == 0.f, "nothing counted: 0 and 0");
    }
    a.d2 = nullptr;          // either output alone selects the joint code
    a.z = nullptr; a.chi2 = nullptr; a.nrej = nullptr; a.screened = nullptr; a.grp = nullptr; a.gate = 0.f;
    check(host_innovation(np, a) == 0, "host_innovation logdet only rc");
  }
}

}  // namespace

int main() {
  for (int np : {1, 2, 3, 4, 7, 10}) {
    run(np, 1, 1);
    run(np, 5, 257);
    run(np, 64, 70);       // INNOV_MAX_BANDS
  }
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("sanitize_evidence ok\n");
  return 0;
}
