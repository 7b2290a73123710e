// kf_device.h — gfx950 (MI355X) kernel templates for the KaFKA engine, shared by
// the translation units kf_kernels.hip, kf_analysis7.hip, kf_analysis10.hip and
// kf_gain10.hip (split so the heavy instantiations compile in parallel, _build.py).
//
// Design: every matrix the reference builds is block
// diagonal with n_p x n_p per-pixel blocks, so the whole Gauss-Newton
// analysis (operator + Jacobian, normal equations, Cholesky, convergence
// partial) is one pixel per lane, SoA layout ([param][pixel], coalesced
// 256-B wave loads), grid-stride over pixels, 256-thread workgroups
// (4 wave64 per workgroup).  GP training records are wave-uniform and are
// read through the scalar path (s_load) so they cost no VGPRs/LDS traffic.
// Deterministic reductions: per-block f64 partials, summed in fixed order
// by reduce_partials_kernel.
#pragma once
#include <hip/hip_runtime.h>
#include "kf_core.h"
#include "kf_launch.h"
#include "kf_gp_mfma.h"

namespace kf {

constexpr int BLOCK = 256;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <int BS = BLOCK>
__device__ __forceinline__ void block_partial(double v, double* partials) {
  __shared__ double red[BS / 64];
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) red[wid] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < BS / 64; ++i) s += red[i];
    partials[blockIdx.x] = s;
  }
}

// Both norm partials of a fused two-iteration launch in one reduction pass.
template <int BS = BLOCK>
__device__ __forceinline__ void block_partials2(double v, double v1, double* partials, double* partials1) {
  __shared__ double red[2][BS / 64];
  v = wave_sum(v);
  v1 = wave_sum(v1);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][wid] = v;
    red[1][wid] = v1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0, s1 = 0.0;
#pragma unroll
    for (int i = 0; i < BS / 64; ++i) {
      s += red[0][i];
      s1 += red[1][i];
    }
    if (partials) partials[blockIdx.x] = s;
    if (partials1) partials1[blockIdx.x] = s1;
  }
}

// ---------------------------------------------------------------------------
// Launch scaffolding of the K1 / K1g kernels (AnalysisArgs or GainArgs): the
// visiting order with n_visit / n_visit_dev, dn_out, the two norm partials of
// gn_fused and the LDS staging of the GP tables are written here once; the
// matrix-core kernels below differ in their per-pixel bodies only.  (The two
// thread-per-pixel kernels write their loop out: through a helper of
// wave_tiles' shape analysis_kernel spills a different number of SGPRs.)

// The launch's norm partials: both of a fused two-iteration launch, else one.
template <int BS = BLOCK, typename A>
__device__ __forceinline__ void launch_partials(const A& a, double acc, double acc1) {
  if (a.partials_first) block_partials2<BS>(acc, acc1, a.partials, a.partials_first);
  else if (a.partials) block_partial<BS>(acc, a.partials);
}

#if defined(__HIP_DEVICE_COMPILE__)
// Every band's split-f16 table into LDS, back to back, the shared zero
// fragment in the last slot (a.gpm_frags - 1), then the workgroup's barrier.
// n_bands: a.n_bands, or a constant so that the band loop unrolls.
template <int BS, int D, typename A>
__device__ __forceinline__ void stage_tables(const A& a, int n_bands, kf_h8* gpm_lds) {
  int off = 0;
  for (int bi = 0; bi < n_bands; ++bi) {
    const KF_CONST_AS BandDesc* bd = cptr(a.bands) + bi;
    const int n = bd->gpm_nchunk * gpm_frags_per_chunk(D);
    const kf_h8* src = (const kf_h8*)bd->gpm;
    for (int i = threadIdx.x; i < n; i += BS) gpm_lds[off + i] = src[i];
    off += n;
  }
  if (threadIdx.x == 0) gpm_lds[a.gpm_frags - 1] = kf_h8{};   // shared zero fragment
  __syncthreads();
}

// The walk of the matrix-core kernels: each wave takes 64 visiting slots at a
// time, grid-stride, and all 64 lanes call f(p, act, dn1) -> dn (the GP sums
// are wave-cooperative).  act = false for the tail lanes past the visit count:
// they run on the last slot's pixel, store nothing and add nothing.
template <int BS, typename A, typename F>
__device__ __forceinline__ void wave_tiles(const A& a, double& acc, double& acc1, F&& f) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * BS;
  const int64_t nv = visit_count(a);
  for (int64_t base = (int64_t)blockIdx.x * BS + (threadIdx.x - lane); base < nv; base += stride) {
    const int64_t q = base + lane;
    const bool act = q < nv;
    const int64_t p = visit_px(a.order, act ? q : nv - 1);
    float dn1;
    const float dn = f(p, act, dn1);
    acc += act ? (double)dn : 0.0;
    acc1 += act ? (double)dn1 : 0.0;
  }
}

// AnalysisArgs.dn_out of an active lane (K1g stores it in gain_pixel's tail).
__device__ __forceinline__ void store_dn_out(int64_t p, bool act, float dn) {
  // re-read through the opaque kernarg pointer: not pinned in SGPRs across the GP loop
  float* dno = opaque((const KF_CONST_AS AnalysisArgs*)__builtin_amdgcn_kernarg_segment_ptr())->dn_out;
  if (act && dno) KF_PX(dno, 0, p) = dn;
}
#endif

template <int NP, int FD = 0, int FOBS = 0, int UNR = 4, bool FOLD = false>
__global__ __launch_bounds__(BLOCK) void analysis_kernel(AnalysisArgs a) {
  double acc = 0.0, acc1 = 0.0;
  const int64_t stride = (int64_t)gridDim.x * BLOCK;
  const int64_t nv = visit_count(a);
  for (int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x; q < nv; q += stride) {
    float dn1;
    const int64_t p = visit_px(a.order, q);
    const float dn = pixel_analysis<NP, FD, FOBS, UNR, FOLD>(a, p, dn1);
    if (a.dn_out) a.dn_out[p] = dn;
    acc += (double)dn;
    acc1 += (double)dn1;
  }
  launch_partials(a, acc, acc1);
}

// K1 with the GP on the matrix cores (kf_gp_mfma.h).  Every band's split-f16
// table is staged in LDS once per workgroup (a.gpm_frags x 16 B of dynamic
// LDS), then each wave walks 64-pixel tiles grid-stride.  BS = 512 with
// MINW = 4 waves per SIMD (<= 128 VGPRs, 2 workgroups per CU for two bands'
// tables) lets the HBM phases (state loads, result stores) of some waves run
// under the record loops of others; BS = 256 gives 3 waves per SIMD.
// The kernel's body is a function of its own with gpm_exp_split's MIXLO flag:
// analysis_mfma_kernel (the default split; its template signature is what
// tests/test_isa_lint.py names) and analysis_mfma_mixlo_kernel
// (AV_MIXLO_SPLIT) are the two kernels around it.
template <int NP, int D, int FOBS, int BS, int LAYOUT, bool IL, int SPEC, bool MIXLO>
__device__ __forceinline__ void analysis_mfma_body(const AnalysisArgs& a) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ kf_h8 gpm_lds[];
  KF_PHASE_KERNEL_BEGIN
  stage_tables<BS, D>(a, a.n_bands, gpm_lds);
  KF_PHASE(KF_PH_PROLOGUE)
  double acc = 0.0, acc1 = 0.0;
  if constexpr (spec_base(SPEC) == SPEC_PROP_PF) {
    // small emulators (short GP loops): the next pixel group's index and its
    // single propagated parameter's x_a / P_a,jj are loaded before this group's
    // analysis, so the forecast starts from registers instead of a dependent
    // order -> state load chain (pixel indices < 2^31: one VGPR carried).
    // wave_tiles' walk with that read-ahead carried across its iterations.
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * BS;
    const int64_t nv = visit_count(a);
    const KF_CONST_AS PropArgs* pa = cptr(a.prop);
    const int pj = prop_single(pa->prop_mask);
    int64_t base = (int64_t)blockIdx.x * BS + (threadIdx.x - lane);
    uint32_t p32 = base < nv ? (uint32_t)visit_px(a.order, base + lane < nv ? base + lane : nv - 1) : 0u;
    float px = 0.f, pp = 0.f;
    if (pj >= 0 && base < nv) {
      px = KF_PX(pa->x_a, pj * pa->ld, (int64_t)p32);
      pp = KF_PX(pa->p_a, tri(NP, pj, pj) * pa->ld, (int64_t)p32);
    }
    for (; base < nv; base += stride) {
      const int64_t q = base + lane;
      const bool act = q < nv;
      const int64_t p = (int64_t)p32;
      const int64_t bn = base + stride;
      uint32_t pn = 0u;
      float pxn = 0.f, ppn = 0.f;
      if (bn < nv) {
        pn = (uint32_t)visit_px(a.order, bn + lane < nv ? bn + lane : nv - 1);
        if (pj >= 0) {
          pxn = KF_PX(pa->x_a, pj * pa->ld, (int64_t)pn);
          ppn = KF_PX(pa->p_a, tri(NP, pj, pj) * pa->ld, (int64_t)pn);
        }
      }
      float dn1;
      const float dn = pixel_analysis_mfma<NP, D, FOBS, false, false, LAYOUT, IL, SPEC, MIXLO>(
          a, p, act, gpm_lds, dn1 KF_PHASE_ARG, pj, px, pp);
      store_dn_out(p, act, dn);
      acc += act ? (double)dn : 0.0;
      acc1 += act ? (double)dn1 : 0.0;
      p32 = pn;
      px = pxn;
      pp = ppn;
    }
  } else {
    wave_tiles<BS>(a, acc, acc1, [&](int64_t p, bool act, float& dn1) {
      const float dn = pixel_analysis_mfma<NP, D, FOBS, false, false, LAYOUT, IL, SPEC, MIXLO>(a, p, act, gpm_lds,
                                                                                              dn1 KF_PHASE_ARG);
      store_dn_out(p, act, dn);
      return dn;
    });
  }
  launch_partials<BS>(a, acc, acc1);
  KF_PHASE_KERNEL_END
#endif
}

template <int NP, int D, int FOBS, int BS = BLOCK, int MINW = 1, int LAYOUT = BAND_LAYOUT_RUNTIME, bool IL = false,
          int SPEC = SPEC_ANY>
__global__ __launch_bounds__(BS, MINW) void analysis_mfma_kernel(AnalysisArgs a) {
  analysis_mfma_body<NP, D, FOBS, BS, LAYOUT, IL, SPEC, false>(a);
}

template <int NP, int D, int FOBS, int BS = BLOCK, int MINW = 1, int LAYOUT = BAND_LAYOUT_RUNTIME, bool IL = false,
          int SPEC = SPEC_ANY>
__global__ __launch_bounds__(BS, MINW) void analysis_mfma_mixlo_kernel(AnalysisArgs a) {
  analysis_mfma_body<NP, D, FOBS, BS, LAYOUT, IL, SPEC, true>(a);
}

// The straight-line JRC-TIP kernel (kf_gp_mfma.h pixel_analysis_tip_sl): the
// launch shape of kf_core.h tip_sl_shape, its constants in a.tc.  ROWS / OUT:
// TIP_ROWS_* / TIP_OUT_* (stored precision rows, fused output rasters).  Each
// group's own loads (tip_group_load) are issued right after its order index.
template <bool IL, int ROWS, int OUT>
__global__ __launch_bounds__(BLOCK, 3) void analysis_tip_sl_kernel(AnalysisArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ kf_h8 gpm_lds[];
  KF_PHASE_KERNEL_BEGIN
  stage_tables<BLOCK, 4>(a, 2, gpm_lds);
  KF_PHASE(KF_PH_PROLOGUE)
  double acc = 0.0, acc1 = 0.0;
  wave_tiles<BLOCK>(a, acc, acc1, [&](int64_t p, bool act, float& dn1) {
    const KF_CONST_AS AnalysisArgs* ka = opaque((const KF_CONST_AS AnalysisArgs*)__builtin_amdgcn_kernarg_segment_ptr());
    const TipGroup g = tip_group_load<OUT>(&ka->tc, p);
    const float dn = pixel_analysis_tip_sl<IL, ROWS, OUT>(p, act, g, gpm_lds, dn1 KF_PHASE_ARG);
    store_dn_out(p, act, dn);
    return dn;
  });
  launch_partials<BLOCK>(a, acc, acc1);
  KF_PHASE_KERNEL_END
#endif
}

// K1 on the matrix cores with every band's table read from global memory
// (gp_mfma_sums_g): many-band GP states (PROSAIL: ten bands, 358-716 KiB of
// tables) whose tables exceed the LDS.  No LDS, so the waves per SIMD follow
// the VGPR count alone.
// (body and the two kernels around it as analysis_mfma_kernel)
template <int NP, int D, int FOBS, bool PF, bool IL, int SPEC, bool MIXLO>
__device__ __forceinline__ void analysis_mfma_g_body(const AnalysisArgs& a) {
  static_assert(BLOCK / 64 == GPM_G_WAVES, "per-wave LDS transpose buffers of gp_mfma_sums_g_xb");
#if defined(__HIP_DEVICE_COMPILE__)
  KF_PHASE_KERNEL_BEGIN
  double acc = 0.0, acc1 = 0.0;
  wave_tiles<BLOCK>(a, acc, acc1, [&](int64_t p, bool act, float& dn1) {
    const float dn = pixel_analysis_mfma<NP, D, FOBS, true, PF, BAND_LAYOUT_RUNTIME, IL, SPEC, MIXLO>(
        a, p, act, nullptr, dn1 KF_PHASE_ARG);
    store_dn_out(p, act, dn);
    return dn;
  });
  launch_partials(a, acc, acc1);
  KF_PHASE_KERNEL_END
#endif
}

template <int NP, int D, int FOBS, bool PF = false, bool IL = false, int SPEC = SPEC_ANY>
__global__ __launch_bounds__(BLOCK, 2) void analysis_mfma_g_kernel(AnalysisArgs a) {
  analysis_mfma_g_body<NP, D, FOBS, PF, IL, SPEC, false>(a);
}

template <int NP, int D, int FOBS, bool PF = false, bool IL = false, int SPEC = SPEC_ANY>
__global__ __launch_bounds__(BLOCK, 2) void analysis_mfma_g_mixlo_kernel(AnalysisArgs a) {
  analysis_mfma_g_body<NP, D, FOBS, PF, IL, SPEC, true>(a);
}

// K1g with the GP on the matrix cores (JRC-TIP: tables staged in LDS once per
// workgroup, as analysis_mfma_kernel).  3 workgroups per CU (168 VGPRs, 80 B
// of scratch per lane) run 6 % faster than 2 (201 VGPRs, 64 B): tip7 gain
// 24.05 vs 25.52 ms/step (profiles/r6_v25_gain_three_waves_ab.jsonl).
// (body and the two kernels around it as analysis_mfma_kernel)
template <int NP, int D, int FOBS, bool MIXLO>
__device__ __forceinline__ void gain_mfma_body(const GainArgs& a) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ kf_h8 gpm_lds[];
  stage_tables<BLOCK, D>(a, a.n_bands, gpm_lds);
  double acc = 0.0, acc1 = 0.0;
  wave_tiles<BLOCK>(a, acc, acc1, [&](int64_t p, bool act, float& dn1) {
    return pixel_gain_mfma<NP, D, FOBS, false, false, MIXLO>(a, p, act, gpm_lds, dn1);
  });
  launch_partials(a, acc, acc1);
#endif
}

template <int NP, int D, int FOBS>
__global__ __launch_bounds__(BLOCK, 3) void gain_mfma_kernel(GainArgs a) {
  gain_mfma_body<NP, D, FOBS, false>(a);
}

template <int NP, int D, int FOBS>
__global__ __launch_bounds__(BLOCK, 3) void gain_mfma_mixlo_kernel(GainArgs a) {
  gain_mfma_body<NP, D, FOBS, true>(a);
}

// K1g on the matrix cores with every band's table read from global memory
// (the gain form's analysis_mfma_g_kernel): ten PROSAIL bands and the
// multi-sensor state, whose tables exceed the LDS.  2 waves per SIMD by the
// launch bound (the 55-float packed covariance per lane, as the information
// form's packed A; 256 VGPRs, 112 B of scratch per lane).  Both column
// blocks' exponent MFMAs are issued first (gpm_chunk IL, as gpm_il_default for
// 10 parameters): the same register and scratch counts as block by block, and
// 1.2 % (prosail10) and 1.9 % (multisensor) faster in an alternating A/B on
// one box (BENCHMARKS.md).
// (body and the two kernels around it as analysis_mfma_kernel)
template <int NP, int D, int FOBS, bool MIXLO>
__device__ __forceinline__ void gain_mfma_g_body(const GainArgs& a) {
  static_assert(BLOCK / 64 == GPM_G_WAVES, "per-wave LDS transpose buffers of gp_mfma_sums_g_xb");
#if defined(__HIP_DEVICE_COMPILE__)
  double acc = 0.0, acc1 = 0.0;
  wave_tiles<BLOCK>(a, acc, acc1, [&](int64_t p, bool act, float& dn1) {
    return pixel_gain_mfma<NP, D, FOBS, true, true, MIXLO>(a, p, act, nullptr, dn1);
  });
  launch_partials(a, acc, acc1);
#endif
}

template <int NP, int D, int FOBS>
__global__ __launch_bounds__(BLOCK, 2) void gain_mfma_g_kernel(GainArgs a) {
  gain_mfma_g_body<NP, D, FOBS, false>(a);
}

template <int NP, int D, int FOBS>
__global__ __launch_bounds__(BLOCK, 2) void gain_mfma_g_mixlo_kernel(GainArgs a) {
  gain_mfma_g_body<NP, D, FOBS, true>(a);
}

template <int NP, int FD = 0, int FOBS = 0>
__global__ __launch_bounds__(BLOCK) void gain_kernel(GainArgs a) {
  double acc = 0.0, acc1 = 0.0;
  const int64_t stride = (int64_t)gridDim.x * BLOCK;
  const int64_t nv = visit_count(a);
  for (int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x; q < nv; q += stride) {
    float dn1;
    acc += (double)pixel_gain<NP, FD, FOBS>(a, visit_px(a.order, q), dn1);
    acc1 += (double)dn1;
  }
  launch_partials(a, acc, acc1);
}

// MODE < 0: runtime a.mode (prepare / classic: Cholesky-sized registers);
// the streaming sweep and finish passes get instantiations of their own so
// that their occupancy is not set by the prepare path's register count.
template <int NP, int MODE = -1>
__global__ __launch_bounds__(BLOCK) void jacobi_kernel(JacobiArgs a) {
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * BLOCK;
  const int64_t n = a.pn > 0 ? a.pn : a.N;
  if constexpr (MODE == JACOBI_SWEEP1D || MODE == JACOBI_FINISH1D) {
    // whole rows [p0 / w, (p0 + n) / w) of a dense strip (checked by the launcher)
    const uint32_t w = (uint32_t)a.geo.w;
    const uint32_t r0 = (uint32_t)(a.p0 / w), nr = (uint32_t)(n / w);
    const int j0 = __builtin_ctz(a.reg_mask);
    for (uint32_t rr = blockIdx.x; rr < nr; rr += gridDim.x) {
      const uint32_t r = r0 + rr;
      // the finish carries NP values per pixel: 2 pixels per thread keep it at
      // 4 waves per SIMD (<= 128 VGPRs; 4 pixels: 147, 3 waves)
      constexpr int UU = MODE == JACOBI_SWEEP1D ? JACOBI_U : 2;
      for (uint32_t c0 = threadIdx.x; c0 < w; c0 += UU * BLOCK) {
        if constexpr (MODE == JACOBI_SWEEP1D) reg_sweep1d<NP, UU, BLOCK>(a, r, c0, j0);
        else acc += (double)reg_finish1d<NP, UU, BLOCK>(a, r, c0);
      }
    }
  } else if constexpr (MODE == JACOBI_FINISH4) {
    // 4-pixel groups of whole rows (w % 4 == 0 and 16-byte alignment: launcher)
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n / 4; i += stride)
      acc += (double)reg_finish4<NP>(a, a.p0 + 4 * i);
  } else if constexpr (MODE == JACOBI_SWEEP1 || MODE == JACOBI_FINISH1) {
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += JACOBI_U * stride) {
      if constexpr (MODE == JACOBI_SWEEP1) reg_sweep1<NP, JACOBI_U>(a, i, stride, n);
      else acc += (double)reg_finish1<NP, JACOBI_U>(a, i, stride, n);
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
      if constexpr (MODE == JACOBI_SWEEP) acc += (double)pixel_reg_sweep<NP>(a, a.p0 + i);
      else if constexpr (MODE == JACOBI_FINISH) acc += (double)pixel_reg_finish<NP>(a, a.p0 + i);
      else acc += (double)pixel_jacobi<NP>(a, a.p0 + i);
    }
  }
  if (a.partials) block_partial(acc, a.partials);
}

// Every auxiliary per-pixel pass (kf_core.h KF_PIXEL_OP: propagate, invert,
// operator, gp_operator, hessian, unpack, marginal, product, smooth, innovation): one
// pixel per thread, grid-stride, every SoA row read and written coalesced.  The
// pass is the tag OP; its arguments' N is the pixel count.
template <int NP, class OP>
__global__ __launch_bounds__(BLOCK) void pixel_kernel(const typename OP::Args a) {
  const int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x; p < a.N; p += stride) OP::template px<NP>(a, p);
}

// K2 split path (pixel_gp_operator) with the VALU GP of D inputs, UNR record
// pairs per step.  RELOAD: the descriptor's epilogue fields are re-read after
// the record stream (61 instead of 91 VGPRs, 26 instead of 233 SGPR spills at
// D=10).
template <int D, int UNR>
struct OpGpOperator {
  using Args = GpOperatorArgs;
  template <int NP>
  static __device__ __forceinline__ void px(const Args& a, int64_t p) {
    pixel_gp_operator<NP>(a, p, [&](const BandDesc& bd, int b, const float (&xv)[NP], float& H0, float (&hv)[NP]) {
      gp_eval<NP, D, UNR, false, true>(bd, xv, H0, hv, a.bands + b);
    });
  }
};

template <typename T>
__global__ __launch_bounds__(BLOCK) void gather_kernel(const T* src, const int64_t* idx, T* dst, int64_t n,
                                                      int rows, int64_t src_ld, int64_t dst_ld) {
  const int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x; p < n; p += stride) {
    const int64_t s = idx[p];  // s < 0: no source pixel (a warp's uncovered target) -> 0 = no data
    KF_DCHECK(s < src_ld);
    for (int r = 0; r < rows; ++r) dst[r * dst_ld + p] = s >= 0 ? src[r * src_ld + s] : T(0);
  }
}

// ---------------------------------------------------------------------------
// launchers
inline int grid_for(int64_t N, int max_blocks) {
  int64_t g = (N + BLOCK - 1) / BLOCK;
  if (g > max_blocks) g = max_blocks;
  if (g < 1) g = 1;
  return (int)g;
}

// K1 / K1g launch tables.  Which kernel a launch takes is decided by
// analysis_plan / gain_plan (kf_plan.h); the lists below are the
// instantiations that exist, one KF_ROW line each: the kernel's name and its
// template arguments, from which both the plan the line answers to and the
// kernel's address are formed.  Each translation unit builds one table from
// the lists of its state sizes (kf_kernels.hip, kf_analysis7.hip,
// kf_analysis10.hip, kf_gain10.hip), which is what instantiates its kernels.
template <typename A>
struct LaunchRow {
  KernelPlan plan;
  void (*kernel)(A);
};
#define KF_ROW(K, ...) {plan_##K(__VA_ARGS__), K<__VA_ARGS__>},

// any bands (the generic kernel), all-precomputed and all-linear operators
#define KF_K1_ROWS_ANY(NP)                            \
  KF_ROW(analysis_kernel, NP, 0, 0)                   \
  KF_ROW(analysis_kernel, NP, FD_PRECOMP, OBS_DN16)   \
  KF_ROW(analysis_kernel, NP, FD_PRECOMP, OBS_F32)    \
  KF_ROW(analysis_kernel, NP, FD_PRECOMP, OBS_BF16)   \
  KF_ROW(analysis_kernel, NP, FD_PRECOMP, OBS_BF16Y)  \
  KF_ROW(analysis_kernel, NP, FD_LINEAR, OBS_DN16)    \
  KF_ROW(analysis_kernel, NP, FD_LINEAR, OBS_F32)     \
  KF_ROW(analysis_kernel, NP, FD_LINEAR, OBS_BF16)    \
  KF_ROW(analysis_kernel, NP, FD_LINEAR, OBS_BF16Y)
// GP bands of FD inputs each: the VALU kernels and the LDS-table matrix-core
// kernels of the runtime layout, in both exponent orders
#define KF_K1_ROWS_GP(NP, FD, MINW)                                                                \
  KF_ROW(analysis_kernel, NP, FD, OBS_DN16)                                                        \
  KF_ROW(analysis_kernel, NP, FD, OBS_F32)                                                         \
  KF_ROW(analysis_mfma_kernel, NP, FD, OBS_DN16, BLOCK, MINW, BAND_LAYOUT_RUNTIME, false, SPEC_ANY) \
  KF_ROW(analysis_mfma_kernel, NP, FD, OBS_DN16, BLOCK, MINW, BAND_LAYOUT_RUNTIME, true, SPEC_ANY)  \
  KF_ROW(analysis_mfma_kernel, NP, FD, OBS_F32, BLOCK, MINW, BAND_LAYOUT_RUNTIME, false, SPEC_ANY)  \
  KF_ROW(analysis_mfma_kernel, NP, FD, OBS_F32, BLOCK, MINW, BAND_LAYOUT_RUNTIME, true, SPEC_ANY)
// full-state GP bands with the tables in global memory (IL0: gpm_il_default)
#define KF_K1_ROWS_GLOBAL(NP, IL0)                                          \
  KF_ROW(analysis_mfma_g_kernel, NP, NP, OBS_DN16, false, false, SPEC_ANY)  \
  KF_ROW(analysis_mfma_g_kernel, NP, NP, OBS_DN16, false, true, SPEC_ANY)   \
  KF_ROW(analysis_mfma_g_kernel, NP, NP, OBS_DN16, false, true, SPEC_PROP)  \
  KF_ROW(analysis_mfma_g_kernel, NP, NP, OBS_DN16, true, false, SPEC_ANY)   \
  KF_ROW(analysis_mfma_g_kernel, NP, NP, OBS_F32, false, IL0, SPEC_ANY)
// the JRC-TIP layout (two 4-input bands, LDS tables)
#define KF_K1_ROWS_TIP_SPEC(K, SPEC) KF_ROW(K, 7, 4, OBS_DN16, BLOCK, 3, BAND_LAYOUT_TIP, true, SPEC)
#define KF_K1_ROWS_TIP                                                                   \
  KF_ROW(analysis_mfma_kernel, 7, 4, OBS_DN16, BLOCK, 3, BAND_LAYOUT_TIP, false, SPEC_ANY) \
  KF_ROW(analysis_mfma_kernel, 7, 4, OBS_F32, BLOCK, 3, BAND_LAYOUT_TIP, false, SPEC_ANY)  \
  KF_ROW(analysis_mfma_kernel, 7, 4, OBS_F32, BLOCK, 3, BAND_LAYOUT_TIP, true, SPEC_ANY)   \
  KF_K1_ROWS_TIP_SPEC(analysis_mfma_kernel, SPEC_ANY)                                    \
  KF_K1_ROWS_TIP_SPEC(analysis_mfma_kernel, SPEC_PROP)                                   \
  KF_K1_ROWS_TIP_SPEC(analysis_mfma_kernel, SPEC_PROP_REG)                               \
  KF_K1_ROWS_TIP_SPEC(analysis_mfma_kernel, SPEC_PROP_PF)                                \
  KF_K1_ROWS_TIP_SPEC(analysis_mfma_kernel, SPEC_PROP_TIP)                               \
  KF_K1_ROWS_TIP_SPEC(analysis_mfma_kernel, SPEC_PROP_REG_TIP)                           \
  KF_K1_ROWS_TIP_SPEC(analysis_mfma_kernel, SPEC_PROP_PF_TIP)                            \
  KF_K1_ROWS_TIP_SPEC(analysis_mfma_mixlo_kernel, SPEC_ANY)                              \
  KF_K1_ROWS_TIP_SPEC(analysis_mfma_mixlo_kernel, SPEC_PROP_TIP)                         \
  KF_K1_ROWS_TIP_SPEC(analysis_mfma_mixlo_kernel, SPEC_PROP_PF_TIP)                      \
  KF_ROW(analysis_tip_sl_kernel, true, TIP_ROWS_NONE, TIP_OUT_NONE)                      \
  KF_ROW(analysis_tip_sl_kernel, true, TIP_ROWS_NONE, TIP_OUT_UNC)                       \
  KF_ROW(analysis_tip_sl_kernel, true, TIP_ROWS_NONE, TIP_OUT_MEAN)                      \
  KF_ROW(analysis_tip_sl_kernel, true, TIP_ROWS_DIAG, TIP_OUT_NONE)                      \
  KF_ROW(analysis_tip_sl_kernel, true, TIP_ROWS_DIAG, TIP_OUT_UNC)                       \
  KF_ROW(analysis_tip_sl_kernel, true, TIP_ROWS_DIAG, TIP_OUT_MEAN)                      \
  KF_ROW(analysis_tip_sl_kernel, true, TIP_ROWS_ALL, TIP_OUT_NONE)                       \
  KF_ROW(analysis_tip_sl_kernel, true, TIP_ROWS_ALL, TIP_OUT_UNC)                        \
  KF_ROW(analysis_tip_sl_kernel, true, TIP_ROWS_ALL, TIP_OUT_MEAN)

// the tables' lists by state size: full-state GPs for small states, JRC-TIP
// (7 params, 4-input band GPs), PROSAIL (10 params, full-state GPs)
#define KF_K1_ROWS_SMALL(NP) KF_K1_ROWS_ANY(NP) KF_K1_ROWS_GP(NP, NP, 3)
#define KF_K1_ROWS_7 \
  KF_K1_ROWS_ANY(7) KF_K1_ROWS_GP(7, 4, 3) KF_K1_ROWS_GP(7, 7, 3) KF_K1_ROWS_GLOBAL(7, false) KF_K1_ROWS_TIP
#define KF_K1_ROWS_10                                                              \
  KF_K1_ROWS_ANY(10) KF_K1_ROWS_GP(10, 10, 1) KF_K1_ROWS_GLOBAL(10, true)          \
  KF_ROW(analysis_mfma_g_mixlo_kernel, 10, 10, OBS_DN16, false, true, SPEC_ANY)    \
  KF_ROW(analysis_mfma_g_mixlo_kernel, 10, 10, OBS_DN16, false, true, SPEC_PROP)

#define KF_K1G_ROWS_SMALL(NP) KF_ROW(gain_kernel, NP, 0, 0)
#define KF_K1G_ROWS_GP(NP, FD) \
  KF_K1G_ROWS_SMALL(NP) KF_ROW(gain_kernel, NP, FD, OBS_DN16) KF_ROW(gain_kernel, NP, FD, OBS_F32)
#define KF_K1G_ROWS_7                            \
  KF_K1G_ROWS_GP(7, 4)                           \
  KF_ROW(gain_mfma_kernel, 7, 4, OBS_DN16)       \
  KF_ROW(gain_mfma_kernel, 7, 4, OBS_F32)        \
  KF_ROW(gain_mfma_mixlo_kernel, 7, 4, OBS_DN16)
#define KF_K1G_ROWS_10                              \
  KF_K1G_ROWS_GP(10, 10)                            \
  KF_ROW(gain_mfma_g_kernel, 10, 10, OBS_DN16)      \
  KF_ROW(gain_mfma_g_kernel, 10, 10, OBS_F32)       \
  KF_ROW(gain_mfma_g_mixlo_kernel, 10, 10, OBS_DN16)

// Launch of the table's kernel for a plan, hipErrorInvalidValue where it has
// none (PLAN_NONE included), on the static grid-stride mapping: norm partials
// per workgroup (grid entries); the hardware dispatcher hands a finished
// workgroup's slot to the next one, which balances the cloud-skip load.
// Round 5's persistent tile queue with per-XCD counters measured within
// 0.5 % of it at 10980^2, 3882^2 and for PROSAIL and was removed in round 6.
template <typename A, size_t N>
static hipError_t launch_plan(const LaunchRow<A> (&rows)[N], const KernelPlan& p, const A& a, int grid,
                              hipStream_t s) {
  for (const LaunchRow<A>& r : rows) {
    if (!(r.plan == p)) continue;
    const size_t lds = plan_lds_tables(p) ? (size_t)a.gpm_frags * sizeof(kf_h8) : 0;
    // dynamic LDS above the 64 KiB default (tables of several bands, up to the
    // 160 KiB of a gfx950 CU)
    if (lds > 64 * 1024)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(r.kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds);
    hipLaunchKernelGGL(r.kernel, dim3(grid), dim3(p.bs), lds, s, a);
    return hipGetLastError();
  }
  return hipErrorInvalidValue;
}

template <typename A, size_t N>
static void table_plans(const LaunchRow<A> (&rows)[N], std::vector<KernelPlan>& out) {
  for (const LaunchRow<A>& r : rows) out.push_back(r.plan);
}

}  // namespace kf
