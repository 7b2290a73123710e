// kf_gp_operator_f64.hip — K2, the split path's GP operator, in float64 on the
// FP64 matrix cores (v_mfma_f64_16x16x4_f64): gp_operator_f64_kernel<NK>, NK in
// {1, 2, 3} K steps of 4 inputs, for every input count 1 <= D <= 10 (D is a
// kernel argument; input slots past D are zero).  The emulator's value and
// Jacobian are float64 from the centred inputs to the epilogue and are rounded
// to float32 once, on the store, so the error is relative to the result and not
// to the cancelling terms (kf_gp_operator_mfma.hip: split f16, f32 sums).  The
// semantics are pixel_gp_operator's (kf_core.h), as K2m states them: per band
// decode_obs, +0.0 in h0 and every state row where the band is masked, the
// gradient scattered through the band's state map, nothing written past N.
//
// Work split: K2m's.  blockIdx.y is the band, blockIdx.x walks groups of BLOCK
// pixels grid-stride, one 64-pixel tile per wave (lane = pixel for the own
// state, the epilogue and the stores; lanes past N run on pixel N - 1 with act =
// false).  One grid per distinct NK of the table; the other bands' workgroups
// leave at once.  A wave none of whose lanes observes the band skips the groups.
//
// Per group of 16 training points and 16-pixel column tile (four tiles per wave
// share the group's A operands):
//   exponent GEMM  E[i][p] = L'_i + c_p + sum_d B_id xi_pd: NK MFMAs whose C
//     operand starts at L'_i + c_p.  The B operand is loaded straight from the
//     SoA state rows: lane l holds input 4 kk + l / 16 of pixel 16 t + l % 16,
//     centred in float64.  c_p = -1/2 log2e sum lambda xi^2 comes from the lane
//     that owns the pixel, read across lanes once per pixel group.
//   m = 2^E (kexp2_f64) on the four accumulator values.
//   sums GEMM  S[f][p] += sum_i A[f][i] m[i][p]: four MFMAs; accumulator
//     register r of the exponent result is MFMA r's B operand as it stands.
// The instruction's layouts (A: row l % 16, k = l / 16; B: k = l / 16, column
// l % 16; D: register r of lane l is row 4 r + l / 16, column l % 16) enter in
// one place, the host table (models/gp.py f64_tables): the point whose exponent
// lands in register r of lane block k is the one whose row constant sits at
// 4 k + r and whose fields are column k of sums operand r, and field f is row f
// of the sums operand.  The kernel only assumes column = l % 16 on both sides.
//
// Data movement.  The band's table is the same for every workgroup of the band
// and small (D = 4, T = 512: 86 KiB), so the operands are read from global
// memory, 8 bytes per lane and coalesced, one group ahead of the MFMAs
// (gp_hessian_sums' register double buffer); the loop waits on the exponential's
// VALU work.  LDS serves the extraction only: after the last group a lane writes
// its 16 sums to its wave's buffer and reads back the D + 1 fields of its own
// pixel, under wave barriers.
#include <algorithm>
#include "kf_device.h"

namespace kf {

typedef double kf_d4 __attribute__((ext_vector_type(4)));

constexpr int GPF_LDS_ROW = 66;   // doubles per field row of a wave's buffer: 64 pixels + 2, so the four lane
                                  // blocks of a store (rows 4 r + k) start in different banks

template <int NK>
struct GpfGroup {                 // one 16-point group's operands of a lane
  double ea[NK];
  kf_d4 lc;
  double sa[4];
};

template <int NK>
__device__ __forceinline__ GpfGroup<NK> gpf_load(const double* tab, int g, int lane) {
  const double* q = tab + GPF_HEADER + (int64_t)g * gpf_group_doubles(NK);
  GpfGroup<NK> o;
#pragma unroll
  for (int kk = 0; kk < NK; ++kk) o.ea[kk] = q[64 * kk + lane];
  o.lc = *(const kf_d4*)(q + 64 * NK + 4 * (lane >> 4));
#pragma unroll
  for (int r = 0; r < 4; ++r) o.sa[r] = q[64 * NK + 16 + 64 * r + lane];
  return o;
}

template <int NK>
__global__ __launch_bounds__(BLOCK, 2) void gp_operator_f64_kernel(const GpOperatorF64Args) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int DS = 4 * NK;                      // input slots
  constexpr double LOG2E_D = 1.4426950408889634, LN2_D = 0.6931471805599453;
  __shared__ double lds[BLOCK / 64][16 * GPF_LDS_ROW];
  const KF_CONST_AS GpOperatorF64Args* ka = (const KF_CONST_AS GpOperatorF64Args*)__builtin_amdgcn_kernarg_segment_ptr();
  const int b = blockIdx.y;
  const int D = ka->d[b];
  if (gpf_k_steps(D) != NK) return;               // another launch's band (workgroup-uniform)
  const KF_CONST_AS BandDesc* bdp = cptr(ka->g.bands) + b;
  const double* tab = ka->tab[b];
  const KF_CONST_AS double* hdr = cptr(tab);
  const int ng = ka->n_groups[b];
  KF_DCHECK(ng >= 1 && D >= 1 && D <= DS && ka->g.nb <= GPO_MAX_BANDS);
  const int64_t N = ka->g.N, ld = ka->g.ld;
  const int tid = threadIdx.x, lane = tid & 63, lk = lane >> 4, lc = lane & 15, wv = tid >> 6;
  double* buf = lds[wv];

  // the input slots 4 kk + lk of the lane's B operands: state row (-1 past D) and centre
  int mrow[NK];
  double cen[NK];
#pragma unroll
  for (int kk = 0; kk < NK; ++kk) {
    const int slot = 4 * kk + lk;
    mrow[kk] = slot < D ? ka->g.bands[b].map[slot] : -1;
    cen[kk] = tab[GPF_CENTER + slot];
  }

  for (int64_t g0 = (int64_t)blockIdx.x * BLOCK; g0 < N; g0 += (int64_t)gridDim.x * BLOCK) {
    const int64_t q = g0 + tid;
    const bool act = q < N;
    const int64_t p = act ? q : N - 1;
    float y, w;
    decode_obs<0>(*bdp, p, y, w);
    const bool use = act && w > 0.f;
    const uint64_t um = __ballot(use);            // wave-uniform: a wave under cloud skips the groups
    // the lane's own centred inputs; zero where it does not use the band: finite operands whatever its state holds
    auto inputs = [&](double (&xi)[DS]) __attribute__((always_inline)) {
#pragma unroll
      for (int d = 0; d < DS; ++d)
        xi[d] = use && d < D ? (double)ka->g.x[(int64_t)bdp->map[d] * ld + p] - hdr[GPF_CENTER + d] : 0.0;
    };
    // masked or unobserved: +0.0 in h0 and every state row
    float H0 = 0.f, gr[DS];
#pragma unroll
    for (int d = 0; d < DS; ++d) gr[d] = 0.f;
    if (um != 0) {
      double c = 0.0;
      {
        double xi[DS];
        inputs(xi);
#pragma unroll
        for (int d = 0; d < DS; ++d) c = __builtin_fma(hdr[GPF_LAM + d] * xi[d], xi[d], c);
        c *= -0.5 * LOG2E_D;
      }
      // B operands and exponent constants of the four column tiles
      double xb[4][NK], cp[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int j = 16 * t + lc;                // the wave's pixel this lane's column is
        const int64_t pj = std::min<int64_t>(g0 + 64 * wv + j, N - 1);
        const bool uj = (um >> j) & 1;
        cp[t] = __shfl(c, j);
#pragma unroll
        for (int kk = 0; kk < NK; ++kk)
          xb[t][kk] = uj && mrow[kk] >= 0 ? (double)ka->g.x[(int64_t)mrow[kk] * ld + pj] - cen[kk] : 0.0;
      }
      kf_d4 acc[4] = {};
      GpfGroup<NK> cur = gpf_load<NK>(tab, 0, lane);
      for (int g = 0; g < ng; ++g) {
        const GpfGroup<NK> nxt = gpf_load<NK>(tab, g + 1 < ng ? g + 1 : g, lane);   // one group ahead
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          kf_d4 e = cur.lc + cp[t];
#pragma unroll
          for (int kk = 0; kk < NK; ++kk) e = __builtin_amdgcn_mfma_f64_16x16x4f64(cur.ea[kk], xb[t][kk], e, 0, 0, 0);
#pragma unroll
          for (int r = 0; r < 4; ++r)
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur.sa[r], kexp2_f64(e[r]), acc[t], 0, 0, 0);
        }
        cur = nxt;
      }
      // extraction: register r of lane block lk is field 4 r + lk of pixel 16 t + lc
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) buf[(4 * r + lk) * GPF_LDS_ROW + 16 * t + lc] = acc[t][r];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (use) {
        double xi[DS];
        inputs(xi);
        const double sc = hdr[0], S0 = buf[lane];
        H0 = (float)(hdr[1] + sc * S0);
#pragma unroll
        for (int d = 0; d < DS; ++d)
          if (d < D) gr[d] = (float)(sc * (LN2_D * buf[(1 + d) * GPF_LDS_ROW + lane] - hdr[GPF_LAM + d] * xi[d] * S0));
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();            // the buffer is free for the next pixel group
    }
    if (act) {
      const int np = ka->np;
      const int64_t ldh = ka->g.ldh;
      const bool ident = bdp->map_identity;
      ka->g.h0[b * ldh + p] = H0;
      float* hrow = ka->g.h + (int64_t)b * np * ldh + p;
      for (int j = 0; j < np; ++j) {
        float v = 0.f;
#pragma unroll
        for (int d = 0; d < DS; ++d) {
          if (ident) v = d == j ? gr[d] : v;
          else v += d < D && bdp->map[d] == j ? gr[d] : 0.f;
        }
        hrow[j * ldh] = v;
      }
    }
  }
#endif
}

// the kernels, one per K-step count: gp_operator_f64_plan's plans
#define KF_GP_OPERATOR_F64_ROWS     \
  KF_ROW(gp_operator_f64_kernel, 1) \
  KF_ROW(gp_operator_f64_kernel, 2) \
  KF_ROW(gp_operator_f64_kernel, 3)
static const LaunchRow<GpOperatorF64Args> gp_operator_f64_rows[] = {KF_GP_OPERATOR_F64_ROWS};

// Workgroups of one launch over all its bands: four rounds of the 2 x 256 that a
// 256-CU device holds at once; set_max_blocks caps it.
constexpr int GPF_GRID = 2048;

hipError_t dev_gp_operator_f64(const std::vector<KernelPlan>& plans, const GpOperatorF64Args& a, hipStream_t s) {
  const GpOperatorArgs& g = a.g;
  if (plans.empty() || g.nb < 1 || g.nb > GPO_MAX_BANDS || g.N > g.ld || g.N > g.ldh || !g.bands || !g.x || !g.h0 ||
      !g.h || !plan_np(a.np))
    return hipErrorInvalidValue;
  // every band belongs to exactly one of the plans, with a table
  for (int b = 0; b < g.nb; ++b) {
    bool found = false;
    for (const KernelPlan& p : plans)
      found = found || (p.family == PLAN_GP_OPERATOR_F64 && gpf_d(a.d[b]) && p.fd == gpf_k_steps(a.d[b]));
    if (!found || !a.tab[b] || a.n_groups[b] < 1 || a.d[b] > a.np) return hipErrorInvalidValue;
  }
  if (g.N <= 0) return hipSuccess;
  const int64_t groups = (g.N + BLOCK - 1) / BLOCK;
  const int cap = std::max(1, std::min(GPF_GRID, get_max_blocks()) / g.nb);
  const int gx = (int)std::min<int64_t>(groups, cap);
  for (const KernelPlan& p : plans) {
    bool launched = false;
    for (const LaunchRow<GpOperatorF64Args>& r : gp_operator_f64_rows) {
      if (!(r.plan == p)) continue;
      hipLaunchKernelGGL(r.kernel, dim3(gx, g.nb), dim3(p.bs), 0, s, a);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
      launched = true;
    }
    if (!launched) return hipErrorInvalidValue;
  }
  return hipSuccess;
}

void launch_table_gp_operator_f64(std::vector<KernelPlan>& out) { table_plans(gp_operator_f64_rows, out); }

}  // namespace kf
