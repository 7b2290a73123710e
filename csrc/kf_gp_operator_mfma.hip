// kf_gp_operator_mfma.hip — K2, the split path's GP operator, on the matrix
// cores: gp_operator_mfma_kernel<D> for D in {2, 3, 4, 7, 10}, beside the
// thread-per-pixel pixel_kernel<NP, OpGpOperator<D, UNR>> of kf_kernels.hip.
// The semantics are pixel_gp_operator's (kf_core.h): per band decode_obs, +0.0
// in h0 and every state row where the band is masked, the emulator's value and
// its input gradient scattered through the band's state map where it is
// observed, nothing written past N.  A translation unit of its own (compiled in
// parallel, _build.py) with a launch table of its own; which launch takes it is
// gp_operator_plan's decision (kf_plan.h).
//
// Work split.  There is no per-pixel linear algebra here, only the two GEMMs of
// kf_gp_mfma.h over one band's table, so the bands are in the grid:
// blockIdx.y is the band, blockIdx.x walks groups of BLOCK pixels grid-stride,
// one 64-pixel tile per wave (lane = pixel; lanes past N run on pixel N - 1
// with act = false).  A workgroup's band is uniform, so its input count is:
// the host launches one grid per distinct D of the table and the workgroups of
// the other bands leave at once.  The state size is a kernel argument, not a
// template argument: the lane gathers its D inputs straight from the state rows
// map[d] (no other row is read) and the gradient's scatter walks the state rows
// in a runtime loop, in gp_epilogue's operand order (gpm_epilogue's for an
// identity map), so the stored bits are those kernels'.
//
// Data movement.  All four waves consume the same band's fragments, so the
// table goes through LDS once per workgroup instead of once per wave
// (gp_mfma_sums_g).  Up to GPO_LDS_FRAGS fragments (36 KiB: four workgroups per
// compute unit) the whole table is staged before the walk and stays; a larger
// one streams through two halves of GPO_RING_FRAGS fragments: a chunk has at most
// BLOCK fragments, so under each chunk the waves consume from one half every
// thread fetches one 16-byte fragment of the same chunk of the next half and
// stores it to the other half after the chunk's MFMAs (4 registers in flight, not
// a half), and one barrier per half hands it over (the half written is the one
// every wave left before the previous barrier).  The ring wraps from the last
// half to the first, so the next pixel group starts without a reload.  A wave
// none of whose lanes observes the band skips the MFMAs but not the staging and
// its barriers.  The centred inputs are formed again after the chunks (the same
// loads and subtraction) instead of being held across them.
// Per chunk the arithmetic is gp_mfma_sums' (gpm_operands, gpm_chunk,
// gpm_extract2): the bits models/gp.py mfma_emulate models.
#include <algorithm>
#include "kf_device.h"

namespace kf {

template <int D>
__global__ __launch_bounds__(BLOCK, 4) void gp_operator_mfma_kernel(const GpOperatorMfmaArgs) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int NK = gpm_k_steps(D), NR = gpm_sum_rows(D), FPC = gpm_frags_per_chunk(D);
  constexpr int HC = gpo_ring_chunks(D);          // chunks per ring half
  static_assert(FPC <= BLOCK && 2 * GPO_RING_FRAGS <= GPO_LDS_FRAGS && HC >= 1, "one fragment per thread and chunk");
  __shared__ kf_h8 lds[GPO_LDS_FRAGS + 1];        // + the shared zero fragment
  // the arguments through the kernarg pointer: indexed by the band, held in no SGPRs across the chunks
  const KF_CONST_AS GpOperatorMfmaArgs* ka = (const KF_CONST_AS GpOperatorMfmaArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  const int b = blockIdx.y;
  if (ka->d[b] != D) return;                      // another launch's band (workgroup-uniform)
  const KF_CONST_AS BandDesc* bdp = cptr(ka->g.bands) + b;
  const kf_h8* tab = (const kf_h8*)ka->tab[b];
  const int nch = ka->n_chunks[b];
  KF_DCHECK(nch >= 1 && ka->g.nb <= GPO_MAX_BANDS);
  const bool ring = nch * FPC > GPO_LDS_FRAGS;
  const int hc = ring ? HC : nch;                 // chunks per half (resident: one half, the table)
  const int nh = (nch + hc - 1) / hc;
  const int64_t N = ka->g.N;
  const int tid = threadIdx.x, lane = tid & 63, hl = lane >> 5;

  // the first half (resident: all of it) and the zero fragment
  for (int i = tid; i < hc * FPC; i += BLOCK) lds[i] = tab[i];
  if (tid == 0) lds[GPO_LDS_FRAGS] = kf_h8{};
  __syncthreads();
  int cur = 0;                                    // ring: the half that holds chunks [0, hc) of the next group

  // the lane's sums fragments (gp_mfma_sums): rows not used read the zero fragment with stride 0
  const int cr = gpm_sum_row<D>(lane & 31);
  const bool ls = cr >= 0;
  const int sbase = ls ? 64 * NK + hl * NR + cr : GPO_LDS_FRAGS;
  const int sstep = ls ? FPC : 0, soff = ls ? 2 * NR : 0;
  const float neg1 = gpm_neg1();

  for (int64_t g0 = (int64_t)blockIdx.x * BLOCK; g0 < N; g0 += (int64_t)gridDim.x * BLOCK) {
    const int64_t q = g0 + tid;
    const bool act = q < N;
    const int64_t p = act ? q : N - 1;
    float y, w;
    decode_obs<0>(*bdp, p, y, w);
    const bool use = act && w > 0.f;
    const bool any = __any(use);                  // wave-uniform: a wave under cloud skips the chunks
    // centred inputs; the band's centre where the lane does not use the band: finite operands whatever its
    // state holds
    auto inputs = [&](float (&xi)[D]) __attribute__((always_inline)) {
#pragma unroll
      for (int d = 0; d < D; ++d)
        xi[d] = use ? ka->g.x[(int64_t)bdp->map[d] * ka->g.ld + p] - bdp->center[d] : 0.f;
    };
    float cl = 0.f;
    kf_h8 xb[2][NK];
    kf_f16v acc[2] = {};
    if (any) {
      float xi[D], c = 0.f;
      inputs(xi);
#pragma unroll
      for (int d = 0; d < D; ++d) c = fmaf(bdp->coef[d] * xi[d], xi[d], c);
      c *= -0.5f * LOG2E;
      gpm_operands<D>(xi, c, xb, cl);
    }
    for (int h = 0; h < nh; ++h) {
      const int n = (h + 1) * hc <= nch ? hc : nch - h * hc;   // this half's chunks
      const kf_h8* t = lds + (ring ? cur * GPO_RING_FRAGS : 0);
      const kf_h8* st = lds + sbase + (ls && ring ? cur * GPO_RING_FRAGS : 0);
      // ring: the next half (the first one after the last), chunk by chunk under this half's
      int nxc = 0;
      const kf_h8* src = tab;
      kf_h8* dst = lds + (cur ^ 1) * GPO_RING_FRAGS;
      if (ring) {
        const int hn = h + 1 < nh ? h + 1 : 0;
        nxc = (hn + 1) * HC <= nch ? HC : nch - hn * HC;
        src = tab + hn * HC * FPC;
      }
      const int steps = n > nxc ? n : nxc;
      for (int ch = 0; ch < steps; ++ch) {
        const bool fetch = ch < nxc && tid < FPC;
        kf_h8 nx;
        if (fetch) nx = src[ch * FPC + tid];
        if (any && ch < n) {
          kf_h8 ea[NK], sa[2];
#pragma unroll
          for (int kk = 0; kk < NK; ++kk) ea[kk] = t[ch * FPC + 64 * kk + lane];
          sa[0] = st[ch * sstep];
          sa[1] = st[ch * sstep + soff];
          gpm_chunk<D, false, false, false>(ea, sa, xb, neg1, acc);
        }
        if (fetch) dst[ch * FPC + tid] = nx;
      }
      if (ring) {
        __syncthreads();
        cur ^= 1;
      }
    }
    // masked or unobserved: +0.0 in h0 and every state row
    float H0 = 0.f, g[D];
#pragma unroll
    for (int d = 0; d < D; ++d) g[d] = 0.f;
    if (any) {
      float S[D + 1];
      gpm_extract2<D>(acc, S);
      if (use) {
        float xi[D];
        inputs(xi);
        const float sc = ka->scale[b], s = kexp2(cl);
        const float S0 = S[0] * s * sc;
        H0 = bdp->offset + S0;
#pragma unroll
        for (int d = 0; d < D; ++d) g[d] = fmaf(-bdp->coef[d] * xi[d], S0, LN2 * (S[1 + d] * s * sc));
      }
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
        for (int d = 0; d < D; ++d) {
          if (ident) v = d == j ? g[d] : v;
          else v += bdp->map[d] == j ? g[d] : 0.f;
        }
        hrow[j * ldh] = v;
      }
    }
  }
#endif
}

// the kernels, one per input count: gp_operator_plan's plans
#define KF_GP_OPERATOR_ROWS          \
  KF_ROW(gp_operator_mfma_kernel, 2) \
  KF_ROW(gp_operator_mfma_kernel, 3) \
  KF_ROW(gp_operator_mfma_kernel, 4) \
  KF_ROW(gp_operator_mfma_kernel, 7) \
  KF_ROW(gp_operator_mfma_kernel, 10)
static const LaunchRow<GpOperatorMfmaArgs> gp_operator_rows[] = {KF_GP_OPERATOR_ROWS};

// Workgroups of one launch over all its bands: four rounds of the 4 x 256 that
// a 256-CU device holds at once, so a workgroup keeps its table for several
// pixel groups and the cloud skip still balances; set_max_blocks caps it.
constexpr int GPO_GRID = 4096;

hipError_t dev_gp_operator_mfma(const std::vector<KernelPlan>& plans, const GpOperatorMfmaArgs& a, hipStream_t s) {
  const GpOperatorArgs& g = a.g;
  if (plans.empty() || g.nb < 1 || g.nb > GPO_MAX_BANDS || g.N > g.ld || g.N > g.ldh || !g.bands || !g.x || !g.h0 ||
      !g.h || !plan_np(a.np))
    return hipErrorInvalidValue;
  // every band belongs to exactly one of the plans, with a table
  for (int b = 0; b < g.nb; ++b) {
    bool found = false;
    for (const KernelPlan& p : plans) found = found || (p.family == PLAN_GP_OPERATOR_MFMA && p.fd == a.d[b]);
    if (!found || !a.tab[b] || a.n_chunks[b] < 1 || a.d[b] > a.np) return hipErrorInvalidValue;
  }
  if (g.N <= 0) return hipSuccess;
  const int64_t groups = (g.N + BLOCK - 1) / BLOCK;
  const int cap = std::max(1, std::min(GPO_GRID, get_max_blocks()) / g.nb);
  const int gx = (int)std::min<int64_t>(groups, cap);
  for (const KernelPlan& p : plans) {
    bool launched = false;
    for (const LaunchRow<GpOperatorMfmaArgs>& r : gp_operator_rows) {
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

void launch_table_gp_operator(std::vector<KernelPlan>& out) { table_plans(gp_operator_rows, out); }

}  // namespace kf
