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
//
// gp_obs_weight_kernel turns that variance into observation weights: the bands of a date in the grid
// (blockIdx.y; blockIdx.x walks the tiles), per tile a decode of the band's observation (decode_obs, every
// encoding), the two phases above only where the tile holds an observation, and in the finish
// w' = w / (1 + w var) = 1 / (sigma_obs^2 + var), stored with y as the planes of an OBS_F32 band.
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

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ kf_h8 gpv_ld(const __amdgpu_buffer_rsrc_t& rs, int lane, int soff) {
  return __builtin_bit_cast(kf_h8, __builtin_amdgcn_raw_buffer_load_b128(rs, lane * 16, soff, 0));
}

// The lane's own pixel pl: the centred inputs as exponent B operands, the exponent constant c and its low
// part cl; false where an input is not finite (the operands are clamped: the pixel is a column of its own).
// T: GpVarArgs, or a GpObsWeightBand behind the kernarg pointer (map, center, lam).
template <int D, typename T>
__device__ __forceinline__ bool gpv_pixel(const T& t, const float* x, int64_t ld, int64_t pl,
                                          kf_h8 (&xb)[2][gpm_k_steps(D)], float& c, float& cl) {
  // Every k^ of the pixel carries 2^c, c = -1/2 log2e sum lambda x^2 ~ -10: c is formed in
  // float64, and from xh + xl, the inputs as the exponent MFMA multiplies them (gpm_operands
  // splits xs into the same halves), so that its rounding does not land on the whole of sum u^2
  float xs[D];
  double cd = 0.0;
  bool fin = true;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const float xi = x[(int64_t)t.map[d] * ld + pl] - t.center[d];
    fin = fin && finitef(xi);
    _Float16 xh, xl;
    gpm_split16(fminf(fmaxf(xi, -6.0e4f), 6.0e4f), xh, xl);
    xs[d] = (float)xh + (float)xl;
    cd = fma((double)t.lam[d] * (double)xs[d], (double)xs[d], cd);
  }
  cd *= -0.5 * 1.4426950408889634;
  c = (float)cd;
  gpm_operands<D>(xs, c, xb, cl);
  cl = (float)(cd - (double)(float)(_Float16)fmaxf(c, -6.0e4f));   // gpm_operands' ch, c's low part from float64
  return fin;
}

// phase 1: k^ of wave w's chunks (every fourth) into LDS, in B-operand layout
template <int D>
__device__ __forceinline__ void gpv_phase1(const __amdgpu_buffer_rsrc_t& ers, int nch, int w, int lane, float neg1,
                                           const kf_h8 (&xb)[2][gpm_k_steps(D)], kf_h8* kfrag) {
  constexpr int NK = gpm_k_steps(D);
  const kf_f16v zero = {};
  for (int ch = w; ch < nch; ch += 4) {
    kf_h8 ea[NK];
#pragma unroll
    for (int kk = 0; kk < NK; ++kk) ea[kk] = gpv_ld(ers, lane, (ch * NK + kk) * 1024);
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
}

// phase 2: wave w's row groups of u = W^ k^, squared and summed per column block
__device__ __forceinline__ void gpv_phase2(const __amdgpu_buffer_rsrc_t& wrs, int nch, int w, int lane,
                                           const kf_h8* kfrag, float (&su)[2]) {
  const kf_f16v zero = {};
  su[0] = su[1] = 0.f;
  for (int k = 0; k < nch; ++k) {
    if (((k & 4) ? 3 - (k & 3) : (k & 3)) != w) continue;
    const int R = nch - 1 - k;
    const int base = R * (R + 1) * 2048;   // block R (R + 1) / 2 of 4 KiB: the row's blocks follow each other
    const int nstep = 2 * (R + 1);         // (chunk, K half) pairs: step s reads k^ fragments 256 s ..
    kf_h8 ah = gpv_ld(wrs, lane, base), al = gpv_ld(wrs, lane, base + 1024);
    kf_f16v acc0 = zero, acc1 = zero;
    for (int s = 0; s < nstep; ++s) {
      const int nx = base + (s + 1 < nstep ? s + 1 : s) * 2048;   // the last step prefetches itself
      const kf_h8 ahn = gpv_ld(wrs, lane, nx), aln = gpv_ld(wrs, lane, nx + 1024);
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
}

// the partial sums into red [wave][wave half][pixel]: the lane holds, of the rows 4 h + .. of its groups,
// pixel n of both column blocks
__device__ __forceinline__ void gpv_partials(float* red, int w, int lane, const float (&su)[2]) {
  const int h = lane >> 5, n = lane & 31;
  red[(w * 2 + h) * 64 + n] = su[0];
  red[(w * 2 + h) * 64 + 32 + n] = su[1];
}

// wave 0, lane = pixel: the fixed-order sum of the partials and the variance in s units times s
__device__ __forceinline__ float gpv_finish(const float* red, int lane, float c, float cl, bool fin, float signal,
                                            float inv_scale2) {
  float tot = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) tot += red[j * 64 + lane];
  // c below the f16 range: every k^ is zero in float32 (2^cl says so; the clamped operands do not)
  const float r = c > -6.0e4f ? (tot * inv_scale2) * kexp2(2.f * cl) : 0.f;
  return fin ? signal * fmaxf(1.f - r, 0.f) : __builtin_nanf("");
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
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int64_t ntile = (a.N + 63) / 64;
  const float neg1 = gpm_neg1();
  const __amdgpu_buffer_rsrc_t ers =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.etab), (short)0, nch * NK * 1024, 0x00020000);
  const __amdgpu_buffer_rsrc_t wrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.wtab), (short)0, (nch * (nch + 1) / 2) * 4096, 0x00020000);
  KF_DCHECK(nch >= 1 && nch <= GPV_MAX_CHUNKS && a.N >= 1 && a.N <= a.ld);
  for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    // the lane's own pixel: centred inputs and the exponent constant
    const int64_t p = tile * 64 + lane;
    const bool act = p < a.N;
    const int64_t pl = act ? p : a.N - 1;
    kf_h8 xb[2][NK];
    float c, cl;
    const bool fin = gpv_pixel<D>(a, a.x, a.ld, pl, xb, c, cl);
    gpv_phase1<D>(ers, nch, w, lane, neg1, xb, kfrag);
    __syncthreads();
    float su[2];
    gpv_phase2(wrs, nch, w, lane, kfrag, su);
    gpv_partials(red, w, lane, su);
    __syncthreads();
    if (w == 0) {
      const float v = gpv_finish(red, lane, c, cl, fin, a.signal, a.inv_scale2);
      if (act) a.out[p] = v;
    }
    // the next tile's phase 1 writes kfrag only, and its barrier comes before the next write of red
  }
#endif
}

// The same two phases per band of the launch (blockIdx.y; a band of another input count belongs to another
// grid), behind a decode of the band's observation: a tile none of whose pixels is observed stores (y, 0)
// and runs neither phase.  Every lane of the workgroup takes the same branch (the OR is workgroup-wide), so
// the barriers per tile are one or three for all four waves alike.
template <int D>
__global__ void __launch_bounds__(BLOCK) gp_obs_weight_kernel(const GpObsWeightArgs) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int NK = gpm_k_steps(D);
  extern __shared__ kf_h8 gpv_lds[];
  // the arguments through the kernarg pointer: indexed by the band (gp_operator_mfma_kernel)
  const KF_CONST_AS GpObsWeightArgs* ka = (const KF_CONST_AS GpObsWeightArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  const KF_CONST_AS GpObsWeightBand& b = ka->band[blockIdx.y];
  if (b.d != D) return;                                     // another launch's band (workgroup-uniform)
  const int nch = b.nchunk;
  const int64_t N = ka->N, ld = ka->ld;
  kf_h8* kfrag = gpv_lds;
  float* red = (float*)(gpv_lds + nch * GPV_CHUNK_FRAGS);   // the launch's LDS holds its largest table
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int64_t ntile = (N + 63) / 64;
  const float neg1 = gpm_neg1();
  const __amdgpu_buffer_rsrc_t ers =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(b.etab), (short)0, nch * NK * 1024, 0x00020000);
  const __amdgpu_buffer_rsrc_t wrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(b.wtab), (short)0, (nch * (nch + 1) / 2) * 4096, 0x00020000);
  KF_DCHECK(nch >= 1 && nch <= GPV_MAX_CHUNKS && N >= 1 && N <= ld && (int)blockIdx.y < ka->nb);
  for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const int64_t p = tile * 64 + lane;
    const bool act = p < N;
    const int64_t pl = act ? p : N - 1;
    float y, wt;
    gpw_decode(b, pl, y, wt);
    const bool st = act && w == 0;                          // wave 0, lane = pixel, stores; tail lanes do not
    if (!__syncthreads_or(act && wt > 0.f)) {
      if (st) {
        b.y_out[p] = y;
        b.w_out[p] = wt;                                    // +0: no lane of the tile is observed
        if (b.var_out) b.var_out[p] = 0.f;
      }
      continue;
    }
    kf_h8 xb[2][NK];
    float c, cl;
    const bool fin = gpv_pixel<D>(b, ka->x, ld, pl, xb, c, cl);
    gpv_phase1<D>(ers, nch, w, lane, neg1, xb, kfrag);
    __syncthreads();
    float su[2];
    gpv_phase2(wrs, nch, w, lane, kfrag, su);
    gpv_partials(red, w, lane, su);
    __syncthreads();
    if (st) {
      const float v = gpv_finish(red, lane, c, cl, fin, b.signal, b.inv_scale2);
      b.y_out[p] = y;
      b.w_out[p] = gpw_weight(wt, v, fin);
      if (b.var_out) b.var_out[p] = v;
    }
    // red is next written past the next observed tile's first barrier, kfrag past the OR's
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

template <int D>
static hipError_t gpw_launch(const GpObsWeightArgs& a, int grid, size_t lds, hipStream_t s) {
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gp_obs_weight_kernel<D>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(gp_obs_weight_kernel<D>, dim3(grid, a.nb), dim3(BLOCK), lds, s, a);
  return hipGetLastError();
}

hipError_t dev_gp_obs_weight(const GpObsWeightArgs& a, int grid, hipStream_t s) {
  if (a.nb < 1 || a.nb > GPW_MAX_BANDS || a.N > a.ld || !a.x) return hipErrorInvalidValue;
  int nchunk = 0;
  bool d4 = false, d10 = false;
  for (int i = 0; i < a.nb; ++i) {
    const GpObsWeightBand& b = a.band[i];
    if (b.nchunk < 1 || b.nchunk > GPV_MAX_CHUNKS || (b.d != 4 && b.d != 10) || !b.etab || !b.wtab || !b.y_out ||
        !b.w_out)
      return hipErrorInvalidValue;
    // the planes the band's encoding reads (decode_obs)
    const bool planes = b.obs == OBS_DN16 ? b.dn != nullptr
                        : b.obs == OBS_F32 || b.obs == OBS_BF16 ? b.y && b.w
                        : b.obs == OBS_BF16Y && b.y;
    if (!planes) return hipErrorInvalidValue;
    nchunk = b.nchunk > nchunk ? b.nchunk : nchunk;
    d4 = d4 || b.d == 4;
    d10 = d10 || b.d == 10;
  }
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
  // one grid per distinct input count, every grid over all bands: a workgroup of another count's band returns
  const size_t lds = gpv_lds_bytes(nchunk);
  hipError_t e = hipSuccess;
  if (d4) e = gpw_launch<4>(a, grid, lds, s);
  if (d10 && e == hipSuccess) e = gpw_launch<10>(a, grid, lds, s);
  return e;
}

std::vector<const char*> gp_variance_table() {
  return {"gp_variance_kernel<4>", "gp_variance_kernel<10>", "gp_obs_weight_kernel<4>", "gp_obs_weight_kernel<10>"};
}

}  // namespace kf
