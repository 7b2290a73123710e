// kf_gp_variance.hip — GP emulator predictive variance on the gfx950 matrix cores.
//
//   var(x) = s - k(x)^T (K + nugget)^-1 k(x) = s (1 - |W^ k^(x)|^2),
//   K + nugget = L L^T,  k^ = k / s in (0, 1],  W^ = sqrt(s) L^-1 (lower triangular).
// The whitened form, not k^T Q k: float32 k^T Q k loses ten times the smallest
// variance of a JRC-TIP emulator to cancellation, |W^ k^|^2 is a sum of squares.
//
// One workgroup = 4 waves = one 64-pixel tile (two 32-pixel column blocks),
// grid-stride over tiles, one workgroup per compute unit.
//
// Phase 1, k^.  Every wave builds the tile's exponent B operands (lane = pixel,
// gpm_operands) and takes every fourth 32-point chunk: the exponent GEMM of
// kf_gp_mfma.h without weights (E = L_i + c_p + B_i . x_p, L_i = -1/2 log2e
// sum lambda t_i^2), exp2, times 2^14 (so the f16 halves of a small k^ stay
// normal numbers; applied after the exponential, where it is exact -- inside E
// it would cost the near points, E ~ 0, their last bits), split into f16 hi
// (toward zero) and lo.  The exponent MFMA leaves the points of a chunk in its
// accumulator exactly as the next MFMA wants its K slots (kf_gp_mfma.h), so each
// lane stores its 8 values as one B fragment: LDS holds k^ in B-operand layout,
// [chunk][K half][column block][hi | lo][lane], 8 KiB per chunk (128 KiB at
// T = 512), written and read as conflict-free ds_*_b128.
//
// Phase 2, u = W^ k^.  W^ is cut into 32 x 32 blocks, the blocks above the
// diagonal dropped; a 32-row group R needs chunks 0..R.  The groups are dealt
// to the waves in a snake (largest first: 0 1 2 3 3 2 1 0 ...), which balances
// the triangle exactly when there are 8 or 16 groups.  A wave streams its
// group's A fragments (hi, lo; 2 KiB per K half, contiguous along the row of
// blocks) from global memory (L2) through a buffer resource into a register
// double buffer, reads k^ from LDS, and issues per K half and column block the
// three split products hi hi, hi lo, lo hi into the group's 2 x 16 accumulator
// registers; the finished rows are squared and added to a per-lane sum.
//
// Finish.  The 4 waves x 2 wave halves' partial sums meet in LDS and wave 0
// (lane = pixel) adds them in a fixed order and stores
// var = s max(0, 1 - sum u^2 2^(2 cl) / w_scale^2) -- cl: the low part of the
// exponent constant, applied once per pixel.  A pixel with a non-finite input
// gets NaN; it is a column of its own in every MFMA and reaches them clamped, so
// no other pixel sees it.  Tail lanes run on pixel N - 1 and store nothing.
#include "kf_device.h"

namespace kf {

constexpr int GPV_K_LOG2 = 14;            // k^ 2^14 <= 2^14 in f16 (models/gp.py GPV_K_LOG2)
constexpr int GPV_CHUNK_FRAGS = 8 * 64;   // k^ fragments per chunk: 2 K halves x 2 blocks x (hi, lo) x 64 lanes
constexpr int GPV_RED_FLOATS = 4 * 2 * 64;

KF_HD size_t gpv_lds_bytes(int nchunk) { return (size_t)nchunk * GPV_CHUNK_FRAGS * 16 + GPV_RED_FLOATS * 4; }

#if defined(__HIP_DEVICE_COMPILE__)
// gpm_exp_split with the 2^GPV_K_LOG2 shift after the exponential
__device__ __forceinline__ void gpv_exp_split(const kf_f16v& e, int r0, float neg1, kf_h8& mh, kf_h8& ml) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float m0 = __builtin_ldexpf(kexp2(e[r0 + 2 * q]), GPV_K_LOG2);
    const float m1 = __builtin_ldexpf(kexp2(e[r0 + 2 * q + 1]), GPV_K_LOG2);
    const kf_hp2 hp = __builtin_amdgcn_cvt_pkrtz(m0, m1);
    const _Float16 h0 = (_Float16)hp[0], h1 = (_Float16)hp[1];
    mh[2 * q] = h0;
    mh[2 * q + 1] = h1;
    const kf_f2 d = {__builtin_fmaf((float)h0, neg1, m0), __builtin_fmaf((float)h1, neg1, m1)};
    const kf_h2 l = __builtin_convertvector(d, kf_h2);
    ml[2 * q] = l[0];
    ml[2 * q + 1] = l[1];
  }
}
#endif

template <int D>
__global__ void __launch_bounds__(BLOCK) gp_variance_kernel(const GpVarArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int NK = gpm_k_steps(D);
  extern __shared__ kf_h8 gpv_lds[];
  const int nch = a.nchunk;
  kf_h8* kfrag = gpv_lds;
  float* red = (float*)(gpv_lds + nch * GPV_CHUNK_FRAGS);   // [wave][wave half][pixel]
  const int lane = threadIdx.x & 63, h = lane >> 5, n = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int64_t ntile = (a.N + 63) / 64;
  const float neg1 = gpm_neg1();
  const kf_f16v zero = {};
  const __amdgpu_buffer_rsrc_t ers =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.etab), (short)0, nch * NK * 1024, 0x00020000);
  const __amdgpu_buffer_rsrc_t wrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.wtab), (short)0, (nch * (nch + 1) / 2) * 4096, 0x00020000);
  const int vo = lane * 16;
  auto ld = [&](const __amdgpu_buffer_rsrc_t& rs, int soff) {
    return __builtin_bit_cast(kf_h8, __builtin_amdgcn_raw_buffer_load_b128(rs, vo, soff, 0));
  };
  KF_DCHECK(nch >= 1 && nch <= GPV_MAX_CHUNKS && a.N >= 1 && a.N <= a.ld);
  for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    // the lane's own pixel: centred inputs and the exponent constant
    const int64_t p = tile * 64 + lane;
    const bool act = p < a.N;
    const int64_t pl = act ? p : a.N - 1;
    // Every k^ of the pixel carries 2^c, c = -1/2 log2e sum lambda x^2 ~ -10: c is formed in
    // float64, and from xh + xl, the inputs as the exponent MFMA multiplies them (gpm_operands
    // splits xs into the same halves), so that its rounding does not land on the whole of sum u^2
    float xs[D];
    double cd = 0.0;
    bool fin = true;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const float xi = a.x[(int64_t)a.map[d] * a.ld + pl] - a.center[d];
      fin = fin && finitef(xi);
      _Float16 xh, xl;
      gpm_split16(fminf(fmaxf(xi, -6.0e4f), 6.0e4f), xh, xl);
      xs[d] = (float)xh + (float)xl;
      cd = fma((double)a.lam[d] * (double)xs[d], (double)xs[d], cd);
    }
    cd *= -0.5 * 1.4426950408889634;
    const float c = (float)cd;
    kf_h8 xb[2][NK];
    float cl;
    gpm_operands<D>(xs, c, xb, cl);
    cl = (float)(cd - (double)(float)(_Float16)fmaxf(c, -6.0e4f));   // gpm_operands' ch, c's low part from float64

    // phase 1: k^ of this wave's chunks into LDS, in B-operand layout
    for (int ch = w; ch < nch; ch += 4) {
      kf_h8 ea[NK];
#pragma unroll
      for (int kk = 0; kk < NK; ++kk) ea[kk] = ld(ers, (ch * NK + kk) * 1024);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        kf_f16v e = __builtin_amdgcn_mfma_f32_32x32x16_f16(ea[0], xb[i][0], zero, 0, 0, 0);
#pragma unroll
        for (int kk = 1; kk < NK; ++kk) e = __builtin_amdgcn_mfma_f32_32x32x16_f16(ea[kk], xb[i][kk], e, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          kf_h8 mh, ml;
          gpv_exp_split(e, 8 * q, neg1, mh, ml);
          kf_h8* dst = kfrag + ((ch * 2 + q) * 2 + i) * 128 + lane;
          dst[0] = mh;
          dst[64] = ml;
        }
      }
    }
    __syncthreads();

    // phase 2: this wave's row groups of u = W^ k^, squared and summed
    float su[2] = {0.f, 0.f};
    for (int k = 0; k < nch; ++k) {
      if (((k & 4) ? 3 - (k & 3) : (k & 3)) != w) continue;
      const int R = nch - 1 - k;
      const int base = R * (R + 1) * 2048;   // block R (R + 1) / 2 of 4 KiB: the row's blocks follow each other
      const int nstep = 2 * (R + 1);         // (chunk, K half) pairs: step s reads k^ fragments 256 s ..
      kf_h8 ah = ld(wrs, base), al = ld(wrs, base + 1024);
      kf_f16v acc0 = zero, acc1 = zero;
      for (int s = 0; s < nstep; ++s) {
        const int nx = base + (s + 1 < nstep ? s + 1 : s) * 2048;   // the last step prefetches itself
        const kf_h8 ahn = ld(wrs, nx), aln = ld(wrs, nx + 1024);
        const kf_h8* kp = kfrag + s * 256 + lane;
        const kf_h8 kh0 = kp[0], kl0 = kp[64], kh1 = kp[128], kl1 = kp[192];
        // the column blocks alternate: no MFMA reads the accumulator the one before it wrote
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, kh0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, kh1, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, kl0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, kl1, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, kh0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, kh1, acc1, 0, 0, 0);
        ah = ahn;
        al = aln;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        su[0] = fmaf(acc0[r], acc0[r], su[0]);
        su[1] = fmaf(acc1[r], acc1[r], su[1]);
      }
    }
    // the lane holds, of the rows 4 h + .. of its groups, pixel n of both column blocks
    red[(w * 2 + h) * 64 + n] = su[0];
    red[(w * 2 + h) * 64 + 32 + n] = su[1];
    __syncthreads();
    if (w == 0) {
      float tot = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) tot += red[j * 64 + lane];
      // c below the f16 range: every k^ is zero in float32 (2^cl says so; the clamped operands do not)
      const float r = c > -6.0e4f ? (tot * a.inv_scale2) * kexp2(2.f * cl) : 0.f;
      const float v = fin ? a.signal * fmaxf(1.f - r, 0.f) : __builtin_nanf("");
      if (act) a.out[p] = v;
    }
    // the next tile's phase 1 writes kfrag only, and its barrier comes before the next write of red
  }
#endif
}

template <int D>
static hipError_t gpv_launch(const GpVarArgs& a, int grid, hipStream_t s) {
  const size_t lds = gpv_lds_bytes(a.nchunk);
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gp_variance_kernel<D>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(gp_variance_kernel<D>, dim3(grid), dim3(BLOCK), lds, s, a);
  return hipGetLastError();
}

hipError_t dev_gp_variance(const GpVarArgs& a, int grid, hipStream_t s) {
  if (a.nchunk < 1 || a.nchunk > GPV_MAX_CHUNKS || a.N > a.ld || !a.x || !a.out || !a.etab || !a.wtab)
    return hipErrorInvalidValue;
  if (a.N <= 0) return hipSuccess;
  const int64_t ntile = (a.N + 63) / 64;
  if (grid <= 0) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
      return hipErrorInvalidValue;
    grid = cus;
  }
  if (grid > ntile) grid = (int)ntile;
  if (a.d == 4) return gpv_launch<4>(a, grid, s);
  if (a.d == 10) return gpv_launch<10>(a, grid, s);
  return hipErrorInvalidValue;
}

std::vector<const char*> gp_variance_table() { return {"gp_variance_kernel<4>", "gp_variance_kernel<10>"}; }

}  // namespace kf
