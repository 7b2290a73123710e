// VALU issue-cost probe for the GP inner loop's instruction mix on gfx950:
// v_exp_f32, v_cvt_pkrtz_f16_f32, v_fma_mixlo_f16, v_fma_f32, v_pk_add_f32,
// alone and mixed, at 1 / 2 / 3 waves per SIMD (one workgroup per CU, held
// there by a large dynamic LDS request; waves w and w + 4 share a SIMD).
// Also: does one wave's v_exp overlap another wave's plain VALU on the same
// SIMD (a separate transcendental pipe) or do their issue costs add?
// Prints one line per (mode, waves/SIMD): shader cycles per instruction per SIMD.
//
// The lo-half split of m (kf_gp_mfma.h gpm_exp_split): the instructions of
// the two bit-identical alternatives to v_fma_mixlo/mixhi_f16 --
//   v_fma_mix_f32 (f16 source, SGPR -1, f32 addend) + v_cvt_pk_f16_f32
//   v_cvt_f32_f16 + v_sub_f32 + v_cvt_pk_f16_f32
// -- each alone, and the split of 8 values as the loop issues it, with its
// real data flow (8 exp, 4 pkrtz, then the lo halves), as "split" lines in
// SIMD cycles per PAIR of values:
//   split mixlo:   2 exp, 1 pkrtz, 1 mixlo + 1 mixhi            (5 per pair)
//   split mixf32:  2 exp, 1 pkrtz, 2 fma_mix_f32, 1 cvt_pk_f16  (6 per pair)
//   split sub:     2 exp, 1 pkrtz, 2 cvt_f32_f16, 2 sub, 1 cvt_pk_f16 (8)
// alone (every wave the split) and beside MFMAs: the last wave of each SIMD
// issues v_mfma_f32_32x32x16_f16 (4 independent accumulators, as
// issue_overlap_probe.hip) until the split waves have finished.  Every
// measurement is repeated REPS times ("rep").
// Build: hipcc --offload-arch=gfx950 -O3 -o valu_issue_probe valu_issue_probe.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>

typedef float f2 __attribute__((ext_vector_type(2)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f16v __attribute__((ext_vector_type(16)));

#define EXP(r) asm volatile("v_exp_f32 %0, %1" : "+v"(r) : "v"(src));
#define FMA(r) asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(r) : "v"(src), "v"(src2));
#define CVT(r) asm volatile("v_cvt_pkrtz_f16_f32 %0, %1, %2" : "+v"(r) : "v"(src), "v"(src2));
#define MIX(r) asm volatile("v_fma_mixlo_f16 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "+v"(r) : "v"(src), "s"(neg1), "v"(src2));
#define PKA(r) asm volatile("v_pk_add_f32 %0, %1, %2" : "+v"(r) : "v"(p0), "v"(p1));
// f16 source (low half of src), SGPR -1, f32 addend, f32 result
#define MIXF(r) asm volatile("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "+v"(r) : "v"(src), "s"(neg1), "v"(src2));
#define CPK(r) asm volatile("v_cvt_pk_f16_f32 %0, %1, %2" : "+v"(r) : "v"(src), "v"(src2));
#define C16(r) asm volatile("v_cvt_f32_f16 %0, %1" : "+v"(r) : "v"(src));
#define SUB(r) asm volatile("v_sub_f32 %0, %1, %2" : "+v"(r) : "v"(src), "v"(src2));

enum { M_SPLIT_MIXLO = 20, M_SPLIT_MIXF32 = 21, M_SPLIT_SUB = 22 };

// The split of 8 values (4 pairs) with its data flow, in gpm_exp_split's order.
template <int MODE>
__device__ __forceinline__ void split8(const float (&e)[8], float neg1, unsigned (&mh)[4], unsigned (&ml)[4]) {
  float m[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) asm volatile("v_exp_f32 %0, %1" : "=v"(m[i]) : "v"(e[i]));
#pragma unroll
  for (int q = 0; q < 4; ++q)
    asm volatile("v_cvt_pkrtz_f16_f32 %0, %1, %2" : "=v"(mh[q]) : "v"(m[2 * q]), "v"(m[2 * q + 1]));
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if constexpr (MODE == M_SPLIT_MIXLO) {
      asm volatile("v_fma_mixlo_f16 %0, %1, %2, %3 op_sel_hi:[1,0,0]"
                   : "+v"(ml[q]) : "v"(mh[q]), "s"(neg1), "v"(m[2 * q]));
      asm volatile("v_fma_mixhi_f16 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
                   : "+v"(ml[q]) : "v"(mh[q]), "s"(neg1), "v"(m[2 * q + 1]));
    } else if constexpr (MODE == M_SPLIT_MIXF32) {
      float d0, d1;
      asm volatile("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(d0) : "v"(mh[q]), "s"(neg1), "v"(m[2 * q]));
      asm volatile("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
                   : "=v"(d1) : "v"(mh[q]), "s"(neg1), "v"(m[2 * q + 1]));
      asm volatile("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(ml[q]) : "v"(d0), "v"(d1));
    } else {
      float h0, h1, d0, d1;
      asm volatile("v_cvt_f32_f16 %0, %1" : "=v"(h0) : "v"(mh[q]));
      asm volatile("v_cvt_f32_f16_sdwa %0, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1" : "=v"(h1) : "v"(mh[q]));
      asm volatile("v_sub_f32 %0, %1, %2" : "=v"(d0) : "v"(m[2 * q]), "v"(h0));
      asm volatile("v_sub_f32 %0, %1, %2" : "=v"(d1) : "v"(m[2 * q + 1]), "v"(h1));
      asm volatile("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(ml[q]) : "v"(d0), "v"(d1));
    }
  }
}

constexpr int SPLIT_MFMA_CAP = 1 << 16;   // groups of 16 MFMAs: the partner waves stop here at the latest

// MFMA: the last wave of each SIMD issues MFMAs until every split wave of the
// workgroup has finished (a counter in LDS), the others run the split.
template <int MODE, bool MFMA>
__global__ void probe_split(long long* out, int iters, float seed) {
  __shared__ int done;
  const int wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
  const int nsplit = MFMA ? nwave - 4 : nwave;
  float neg1 = -1.0f;
  asm volatile("" : "+s"(neg1));
  if (threadIdx.x == 0) done = 0;
  __syncthreads();
  if (MFMA && wave >= nsplit) {
    h8 a, b;
    for (int i = 0; i < 8; ++i) {
      a[i] = (_Float16)(seed * 1e-3f + i);
      b[i] = (_Float16)(seed * 1e-3f - i);
    }
    f16v acc[4];
    for (int j = 0; j < 4; ++j)
      for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
    for (int k = 0; k < SPLIT_MFMA_CAP; ++k) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc[1], 0, 0, 0);
        acc[2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc[2], 0, 0, 0);
        acc[3] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc[3], 0, 0, 0);
      }
      if (*(volatile int*)&done >= nsplit) break;
    }
    float t = 0.f;
    for (int j = 0; j < 4; ++j) t += acc[j][threadIdx.x & 15];
    if (t == 12345.678f) out[0] = (long long)t;   // keep the MFMAs alive
    return;
  }
  float e[8];
  for (int i = 0; i < 8; ++i) e[i] = seed * 0.25f * i - (float)(threadIdx.x & 7);
  unsigned mh[4] = {0, 0, 0, 0}, ml[4] = {0, 0, 0, 0};
  const long long t0 = clock64();
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int u = 0; u < 4; ++u) split8<MODE>(e, neg1, mh, ml);
  }
  const long long t1 = clock64();
  asm volatile("" ::"v"(mh[0]), "v"(mh[1]), "v"(mh[2]), "v"(mh[3]), "v"(ml[0]), "v"(ml[1]), "v"(ml[2]), "v"(ml[3]));
  if ((threadIdx.x & 63) == 0) {
    out[blockIdx.x * nsplit + wave] = t1 - t0;
    atomicAdd(&done, 1);
  }
}

template <int MODE>
__global__ void probe(long long* out, int iters, float seed) {
  float src = seed + threadIdx.x, src2 = seed * 0.5f;
  float neg1 = -1.0f;
  asm volatile("" : "+s"(neg1));
  f2 p0 = {src, src2}, p1 = {src2, src};
  float r0 = 0, r1 = 0, r2 = 0, r3 = 0, r4 = 0, r5 = 0, r6 = 0, r7 = 0;
  f2 q0 = p0, q1 = p1, q2 = p0, q3 = p1;
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  const long long t0 = clock64();
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if constexpr (MODE == 0) { EXP(r0) EXP(r1) EXP(r2) EXP(r3) EXP(r4) EXP(r5) EXP(r6) EXP(r7) }
      if constexpr (MODE == 1) { MIX(r0) MIX(r1) MIX(r2) MIX(r3) MIX(r4) MIX(r5) MIX(r6) MIX(r7) }
      if constexpr (MODE == 2) { CVT(r0) CVT(r1) CVT(r2) CVT(r3) CVT(r4) CVT(r5) CVT(r6) CVT(r7) }
      if constexpr (MODE == 3) { FMA(r0) FMA(r1) FMA(r2) FMA(r3) FMA(r4) FMA(r5) FMA(r6) FMA(r7) }
      if constexpr (MODE == 4) { PKA(q0) PKA(q1) PKA(q2) PKA(q3) PKA(q0) PKA(q1) PKA(q2) PKA(q3) }
      // exp and fma interleaved in one wave (do their costs add?)
      if constexpr (MODE == 5) { EXP(r0) FMA(r1) EXP(r2) FMA(r3) EXP(r4) FMA(r5) EXP(r6) FMA(r7) }
      // waves 0-3 exp, waves 4-7 (their SIMD partners) fma: separate pipes?
      if constexpr (MODE == 6) {
        if (wave < 4) { EXP(r0) EXP(r1) EXP(r2) EXP(r3) EXP(r4) EXP(r5) EXP(r6) EXP(r7) }
        else { FMA(r0) FMA(r1) FMA(r2) FMA(r3) FMA(r4) FMA(r5) FMA(r6) FMA(r7) }
      }
      // the GP loop's per-value mix: 2 exp, 1 cvt, 2 mix per 2 values
      if constexpr (MODE == 7) { EXP(r0) EXP(r1) CVT(r2) MIX(r3) MIX(r4) EXP(r5) EXP(r6) CVT(r7) }
      // the candidate splits' instructions
      if constexpr (MODE == 8) { MIXF(r0) MIXF(r1) MIXF(r2) MIXF(r3) MIXF(r4) MIXF(r5) MIXF(r6) MIXF(r7) }
      if constexpr (MODE == 9) { CPK(r0) CPK(r1) CPK(r2) CPK(r3) CPK(r4) CPK(r5) CPK(r6) CPK(r7) }
      if constexpr (MODE == 10) { C16(r0) C16(r1) C16(r2) C16(r3) C16(r4) C16(r5) C16(r6) C16(r7) }
      if constexpr (MODE == 11) { SUB(r0) SUB(r1) SUB(r2) SUB(r3) SUB(r4) SUB(r5) SUB(r6) SUB(r7) }
    }
  }
  const long long t1 = clock64();
  asm volatile("" ::"v"(r0), "v"(r1), "v"(r2), "v"(r3), "v"(r4), "v"(r5), "v"(r6), "v"(r7));
  if constexpr (MODE == 4) asm volatile("" ::"v"(q0), "v"(q1), "v"(q2), "v"(q3));
  if ((threadIdx.x & 63) == 0) out[blockIdx.x * (blockDim.x >> 6) + wave] = t1 - t0;
}

constexpr int REPS = 3;
constexpr size_t LDS = 96 * 1024;   // one workgroup per CU

template <int MODE>
static void run(const char* name, int wps, long long* d, int ncu) {
  const int threads = 256 * wps, iters = 4000;
  hipFuncSetAttribute((const void*)probe<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS);
  hipEvent_t a, b;
  hipEventCreate(&a);
  hipEventCreate(&b);
  for (int rep = 0; rep < REPS; ++rep) {
    probe<MODE><<<ncu, threads, LDS>>>(d, 16, 1.0f);
    hipEventRecord(a);
    probe<MODE><<<ncu, threads, LDS>>>(d, iters, 1.0f);
    hipEventRecord(b);
    hipEventSynchronize(b);
    float ms = 0;
    hipEventElapsedTime(&ms, a, b);
    const int nw = ncu * threads / 64;
    std::vector<long long> h(nw);
    hipMemcpy(h.data(), d, nw * sizeof(long long), hipMemcpyDeviceToHost);
    double mean = 0;
    for (auto v : h) mean += (double)v;
    mean /= nw;
    const double insts = (double)iters * 32;
    // waves on one SIMD run concurrently: SIMD cycles per instruction
    const double cpi = mean / (insts * wps);
    const double mhz = mean / (ms * 1e3);
    printf("{\"mode\": \"%s\", \"waves_per_simd\": %d, \"rep\": %d, \"cycles_per_inst_per_simd\": %.2f, "
           "\"wave_cycles\": %.0f, \"kernel_ms\": %.3f, \"clock_mhz_est\": %.0f}\n",
           name, wps, rep, cpi, mean, ms, mhz);
  }
  hipEventDestroy(a);
  hipEventDestroy(b);
}

// wps waves per SIMD in all; with MFMA one of them issues MFMAs and wps - 1 the split
template <int MODE, bool MFMA>
static void run_split(const char* name, int wps, long long* d, int ncu) {
  const int threads = 256 * wps, iters = 2000;
  const int nsplit = MFMA ? wps - 1 : wps;   // split waves per SIMD
  hipFuncSetAttribute((const void*)probe_split<MODE, MFMA>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS);
  hipEvent_t a, b;
  hipEventCreate(&a);
  hipEventCreate(&b);
  for (int rep = 0; rep < REPS; ++rep) {
    probe_split<MODE, MFMA><<<ncu, threads, LDS>>>(d, 16, 1.0f);
    hipEventRecord(a);
    probe_split<MODE, MFMA><<<ncu, threads, LDS>>>(d, iters, 1.0f);
    hipEventRecord(b);
    hipEventSynchronize(b);
    float ms = 0;
    hipEventElapsedTime(&ms, a, b);
    const int nw = ncu * 4 * nsplit;
    std::vector<long long> h(nw);
    hipMemcpy(h.data(), d, nw * sizeof(long long), hipMemcpyDeviceToHost);
    double mean = 0;
    for (auto v : h) mean += (double)v;
    mean /= nw;
    const double pairs = (double)iters * 16;   // 4 split8 of 4 pairs per iteration
    const int per_pair = MODE == M_SPLIT_MIXLO ? 5 : MODE == M_SPLIT_MIXF32 ? 6 : 8;
    printf("{\"mode\": \"%s\", \"beside_mfma\": %s, \"waves_per_simd\": %d, \"split_waves_per_simd\": %d, \"rep\": %d, "
           "\"insts_per_pair\": %d, \"cycles_per_pair_per_simd\": %.2f, \"wave_cycles\": %.0f, \"kernel_ms\": %.3f}\n",
           name, MFMA ? "true" : "false", wps, nsplit, rep, per_pair, mean / (pairs * nsplit), mean, ms);
  }
  hipEventDestroy(a);
  hipEventDestroy(b);
}

int main() {
  int ncu = 0;
  hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, 0);
  long long* d;
  hipMalloc(&d, (size_t)ncu * 16 * sizeof(long long));
  for (int w = 1; w <= 3; ++w) {
    run<0>("exp", w, d, ncu);
    run<1>("fma_mixlo", w, d, ncu);
    run<2>("cvt_pkrtz", w, d, ncu);
    run<3>("fma_f32", w, d, ncu);
    run<4>("pk_add_f32", w, d, ncu);
    run<5>("exp+fma same wave", w, d, ncu);
    if (w >= 2) run<6>("exp waves0-3 | fma waves4-7", w, d, ncu);
    run<7>("gp mix 4exp 2cvt 2mix", w, d, ncu);
    run<8>("fma_mix_f32", w, d, ncu);
    run<9>("cvt_pk_f16_f32", w, d, ncu);
    run<10>("cvt_f32_f16", w, d, ncu);
    run<11>("sub_f32", w, d, ncu);
    run_split<M_SPLIT_MIXLO, false>("split mixlo", w, d, ncu);
    run_split<M_SPLIT_MIXF32, false>("split mixf32", w, d, ncu);
    run_split<M_SPLIT_SUB, false>("split sub", w, d, ncu);
    if (w >= 2) {
      run_split<M_SPLIT_MIXLO, true>("split mixlo", w, d, ncu);
      run_split<M_SPLIT_MIXF32, true>("split mixf32", w, d, ncu);
      run_split<M_SPLIT_SUB, true>("split sub", w, d, ncu);
    }
    fflush(stdout);
  }
  hipFree(d);
  return 0;
}
