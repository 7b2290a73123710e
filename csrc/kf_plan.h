// kf_plan.h — which kernel an analysis (K1) or gain (K1g) launch takes, as a
// plain value computed on the host: no HIP calls, compiled by g++ (bindings)
// and hipcc alike.  analysis_plan / gain_plan are the whole decision; the
// launchers of kf_device.h only look the plan up in their table of the
// instantiations that exist (KF_ROW) and launch it.  A new variant adds one
// line here and one table line; tests/test_launch_plan.py pins every launch.
#pragma once
#include <string>
#include <type_traits>
#include "kf_core.h"

namespace kf {

// The kernel templates of kf_device.h.  PLAN_NONE: no kernel for this launch
// (the caller gets hipErrorInvalidValue).
enum PlanFamily : int {
  PLAN_NONE = 0,
  PLAN_ANALYSIS,             // analysis_kernel<NP>: any bands, the f32 VALU record loop
  PLAN_ANALYSIS_FAST,        // analysis_kernel<NP, FD, OBS>: one operator kind and observation encoding
  PLAN_ANALYSIS_MFMA,        // analysis_mfma_kernel: GP on the matrix cores, tables in LDS
  PLAN_ANALYSIS_MFMA_MIXLO,  // analysis_mfma_mixlo_kernel (AV_MIXLO_SPLIT)
  PLAN_ANALYSIS_MFMA_G,      // analysis_mfma_g_kernel: tables in global memory
  PLAN_ANALYSIS_MFMA_G_MIXLO,
  PLAN_ANALYSIS_TIP_SL,      // analysis_tip_sl_kernel: the straight-line JRC-TIP kernel
  PLAN_GAIN,                 // gain_kernel<NP> and gain_kernel<NP, FD, OBS>
  PLAN_GAIN_MFMA,
  PLAN_GAIN_MFMA_MIXLO,
  PLAN_GAIN_MFMA_G,
  PLAN_GAIN_MFMA_G_MIXLO,
};

constexpr int PLAN_BLOCK = 256;   // kf_device.h BLOCK: every K1 / K1g kernel's workgroup

// One instantiation: the family and its template arguments (those the family
// does not have stay 0).  bs: the workgroup size; mixlo: a *_mixlo_kernel twin.
struct KernelPlan {
  int family = PLAN_NONE;
  int np = 0, fd = 0, obs = 0, bs = 0, minw = 0, layout = 0;
  bool il = false;
  int spec = 0;
  bool mixlo = false, pf = false;
  int rows = 0, out = 0;
};

constexpr bool operator==(const KernelPlan& x, const KernelPlan& y) {
  return x.family == y.family && x.np == y.np && x.fd == y.fd && x.obs == y.obs && x.bs == y.bs &&
         x.minw == y.minw && x.layout == y.layout && x.il == y.il && x.spec == y.spec && x.mixlo == y.mixlo &&
         x.pf == y.pf && x.rows == y.rows && x.out == y.out;
}

// plan_<kernel>(template arguments in the kernel's own order): what KF_ROW
// (kf_device.h) keys a table line with, and what the two choices below return.
constexpr KernelPlan plan_analysis_kernel(int np, int fd, int obs) {
  return {fd == 0 && obs == 0 ? PLAN_ANALYSIS : PLAN_ANALYSIS_FAST, np, fd, obs, PLAN_BLOCK};
}
constexpr KernelPlan plan_analysis_mfma_kernel(int np, int d, int obs, int bs, int minw, int layout, bool il,
                                               int spec) {
  return {PLAN_ANALYSIS_MFMA, np, d, obs, bs, minw, layout, il, spec};
}
constexpr KernelPlan plan_analysis_mfma_mixlo_kernel(int np, int d, int obs, int bs, int minw, int layout, bool il,
                                                     int spec) {
  return {PLAN_ANALYSIS_MFMA_MIXLO, np, d, obs, bs, minw, layout, il, spec, true};
}
constexpr KernelPlan plan_analysis_mfma_g_kernel(int np, int d, int obs, bool pf, bool il, int spec) {
  return {PLAN_ANALYSIS_MFMA_G, np, d, obs, PLAN_BLOCK, 0, 0, il, spec, false, pf};
}
constexpr KernelPlan plan_analysis_mfma_g_mixlo_kernel(int np, int d, int obs, bool pf, bool il, int spec) {
  return {PLAN_ANALYSIS_MFMA_G_MIXLO, np, d, obs, PLAN_BLOCK, 0, 0, il, spec, true, pf};
}
constexpr KernelPlan plan_analysis_tip_sl_kernel(bool il, int rows, int out) {
  return {PLAN_ANALYSIS_TIP_SL, 7, 4, OBS_DN16, PLAN_BLOCK, 0, BAND_LAYOUT_TIP, il, 0, false, false, rows, out};
}
constexpr KernelPlan plan_gain(int family, int np, int fd, int obs, bool mixlo = false) {
  return {family, np, fd, obs, PLAN_BLOCK, 0, 0, false, 0, mixlo};
}
constexpr KernelPlan plan_gain_kernel(int np, int fd, int obs) { return plan_gain(PLAN_GAIN, np, fd, obs); }
constexpr KernelPlan plan_gain_mfma_kernel(int np, int d, int obs) { return plan_gain(PLAN_GAIN_MFMA, np, d, obs); }
constexpr KernelPlan plan_gain_mfma_mixlo_kernel(int np, int d, int obs) {
  return plan_gain(PLAN_GAIN_MFMA_MIXLO, np, d, obs, true);
}
constexpr KernelPlan plan_gain_mfma_g_kernel(int np, int d, int obs) {
  return plan_gain(PLAN_GAIN_MFMA_G, np, d, obs);
}
constexpr KernelPlan plan_gain_mfma_g_mixlo_kernel(int np, int d, int obs) {
  return plan_gain(PLAN_GAIN_MFMA_G_MIXLO, np, d, obs, true);
}

// Kernels with the bands' tables in dynamic LDS (a.gpm_frags fragments of 16 B).
constexpr bool plan_lds_tables(const KernelPlan& p) {
  return p.family == PLAN_ANALYSIS_MFMA || p.family == PLAN_ANALYSIS_MFMA_MIXLO ||
         p.family == PLAN_ANALYSIS_TIP_SL || p.family == PLAN_GAIN_MFMA || p.family == PLAN_GAIN_MFMA_MIXLO;
}

// The plan's template-id as a demangler prints it for the kernel's symbol
// (default template arguments included), "NONE" for PLAN_NONE.
inline std::string plan_name(const KernelPlan& p) {
  const auto b = [](bool v) { return std::string(v ? "true" : "false"); };
  const auto i = [](int v) { return std::to_string(v); };
  const std::string head = i(p.np) + ", " + i(p.fd) + ", " + i(p.obs);
  const std::string mfma = head + ", " + i(p.bs) + ", " + i(p.minw) + ", " + i(p.layout) + ", " + b(p.il) + ", " +
                           i(p.spec) + ">";
  const std::string g = head + ", " + b(p.pf) + ", " + b(p.il) + ", " + i(p.spec) + ">";
  switch (p.family) {
    case PLAN_ANALYSIS:
    case PLAN_ANALYSIS_FAST: return "analysis_kernel<" + head + ", 4, false>";   // UNR, FOLD defaults
    case PLAN_ANALYSIS_MFMA: return "analysis_mfma_kernel<" + mfma;
    case PLAN_ANALYSIS_MFMA_MIXLO: return "analysis_mfma_mixlo_kernel<" + mfma;
    case PLAN_ANALYSIS_MFMA_G: return "analysis_mfma_g_kernel<" + g;
    case PLAN_ANALYSIS_MFMA_G_MIXLO: return "analysis_mfma_g_mixlo_kernel<" + g;
    case PLAN_ANALYSIS_TIP_SL:
      return "analysis_tip_sl_kernel<" + b(p.il) + ", " + i(p.rows) + ", " + i(p.out) + ">";
    case PLAN_GAIN: return "gain_kernel<" + head + ">";
    case PLAN_GAIN_MFMA: return "gain_mfma_kernel<" + head + ">";
    case PLAN_GAIN_MFMA_MIXLO: return "gain_mfma_mixlo_kernel<" + head + ">";
    case PLAN_GAIN_MFMA_G: return "gain_mfma_g_kernel<" + head + ">";
    case PLAN_GAIN_MFMA_G_MIXLO: return "gain_mfma_g_mixlo_kernel<" + head + ">";
    default: return "NONE";
  }
}

// The state sizes with compiled kernels, listed once for both runners:
// f(std::integral_constant<int, NP>) for np's size -> true, false for any other.
template <class F>
constexpr bool np_dispatch(int np, F&& f) {
  switch (np) {
    case 1: f(std::integral_constant<int, 1>{}); return true;
    case 2: f(std::integral_constant<int, 2>{}); return true;
    case 3: f(std::integral_constant<int, 3>{}); return true;
    case 4: f(std::integral_constant<int, 4>{}); return true;
    case 7: f(std::integral_constant<int, 7>{}); return true;
    case 10: f(std::integral_constant<int, 10>{}); return true;
    default: return false;
  }
}
constexpr bool plan_np(int np) { return np_dispatch(np, [](auto) {}); }

// Interleaved exponent MFMAs (gpm_chunk IL: both column blocks' exponent
// MFMAs before the first block's exponentials) by default where the second
// live block costs no waves per SIMD and no scratch (ISA lint,
// tests/test_isa_lint.py): the JRC-TIP layout kernel (156 -> 168 VGPRs, 3
// waves either way) and 10-parameter states (2 waves either way); +0.5% tip7,
// +1.0% prosail10 interleaved on one box (profiles/r4_v2_ab_fixed_tip7T.jsonl).
// Elsewhere (7-parameter runtime layout: 8-24 B scratch; 3-4 parameters: 4 ->
// 3 waves) the block-by-block order stays.
constexpr bool gpm_il_default(int np, int layout) { return (np == 7 && layout == BAND_LAYOUT_TIP) || np >= 10; }

// K1 with the LDS-table matrix-core kernels: split-f16 tables attached to
// every band and small enough for the LDS (ops/kernels.py band_table).
inline KernelPlan analysis_plan_lds(int np, const AnalysisArgs& a) {
  const int fd = a.fast_d, obs = a.fast_obs, v = a.variant;
  // JRC-TIP band layout (AnalysisArgs.band_layout, checked on the host):
  // band loop unrolled over the two compile-time maps (AV_RUNTIME_LAYOUT:
  // the runtime-layout kernel, its oracle)
  const bool tip = np == 7 && fd == 4 && a.band_layout == BAND_LAYOUT_TIP && a.n_bands == 2 && v != AV_RUNTIME_LAYOUT;
  const int layout = tip ? BAND_LAYOUT_TIP : BAND_LAYOUT_RUNTIME;
  // Launch bound of 3 workgroups per CU (MINW = 3, as the LDS tables
  // allow) up to 7 parameters: the compiler holds the kernel to <= 168
  // VGPRs itself (A/B neutral against landing there unconstrained,
  // profiles/r3_v13_*); 10 parameters would spill, so no bound there.
  const int minw = np <= 7 ? 3 : 1;
  // Both column blocks' exponent MFMAs issued before the first block's
  // exponentials (gpm_chunk IL) where that costs no occupancy
  // (gpm_il_default); AV_BLOCK_ORDER: the other order
  const bool il0 = gpm_il_default(np, layout);
  const KernelPlan any =
      plan_analysis_mfma_kernel(np, fd, obs, PLAN_BLOCK, minw, layout, il0 != (v == AV_BLOCK_ORDER), SPEC_ANY);
  if (!tip || obs != OBS_DN16) return any;
  // the launch shape of the straight-line kernel (a.tc filled by the host: tip_const_fill);
  // AV_LOOPED_TIP: the SPEC_PROP_TIP kernels below for the same launch (its oracle)
  if (a.tc.on && v == AV_DEFAULT && a.tc.rows >= TIP_ROWS_NONE && a.tc.rows <= TIP_ROWS_ALL &&
      a.tc.out >= TIP_OUT_NONE && a.tc.out <= TIP_OUT_MEAN)
    return plan_analysis_tip_sl_kernel(il0, a.tc.rows, a.tc.out);
  // JRC-TIP layout with the forecast fused (every date after the first):
  // the launch's paths fixed at compile time (SPEC_PROP / SPEC_PROP_REG,
  // kf_core.h); AV_GENERIC_SPEC: the generic kernel.  With the JRC-TIP zero
  // structure of the forecast precision (AnalysisArgs.a_struct, checked on
  // the host) their SPEC_*_TIP twins with the structure-aware solve;
  // AV_DENSE_SOLVE: the dense kernels all the same
  const bool tips = (a.a_struct & A_STRUCT_TIP) && v != AV_DENSE_SOLVE;
  // small emulators (<= 4 chunks of 32 training points per band): the GP
  // loop is too short to hide the next group's forecast loads, so the
  // SPEC_PROP_PF kernel loads them ahead (T = 32: -2.2 %; at T = 500 the
  // extra registers cost +0.5 %, profiles/r5_forecast_prefetch_ab.jsonl)
  const bool small = a.gpm_frags <= 4 * a.n_bands * gpm_frags_per_chunk(fd) + 1;
  const auto spec = [&](int s) { return plan_analysis_mfma_kernel(np, fd, obs, PLAN_BLOCK, minw, layout, il0, s); };
  // AV_MIXLO_SPLIT is built for the first date's generic launch and the
  // structure-aware fused forecast without a regulariser; any other fused
  // forecast falls to a kernel without the split below (analysis_plan: NONE)
  if (v == AV_MIXLO_SPLIT && (!a.prop || (tips && !a.reg_v)))
    return plan_analysis_mfma_mixlo_kernel(np, fd, obs, PLAN_BLOCK, minw, layout, il0,
                                           !a.prop ? SPEC_ANY : small ? SPEC_PROP_PF_TIP : SPEC_PROP_TIP);
  if (!a.prop || v == AV_BLOCK_ORDER || v == AV_GENERIC_SPEC) return any;
  if (a.reg_v) return spec(tips ? SPEC_PROP_REG_TIP : SPEC_PROP_REG);
  if (small) return spec(tips ? SPEC_PROP_PF_TIP : SPEC_PROP_PF);
  return spec(tips ? SPEC_PROP_TIP : SPEC_PROP);
}

// K1 on the matrix cores with the tables read from global memory: full-state
// GP bands (FD == NP) of 7- and 10-parameter states whose tables exceed the LDS.
inline KernelPlan analysis_plan_global(int np, const AnalysisArgs& a) {
  const int fd = a.fast_d, v = a.variant;
  const bool il0 = gpm_il_default(np, BAND_LAYOUT_RUNTIME);
  if (a.fast_obs == OBS_F32) return plan_analysis_mfma_g_kernel(np, fd, OBS_F32, false, il0, SPEC_ANY);
  // AV_GT_PREFETCH: register double buffer (next chunk's fragments
  // loaded under the current one): 191.7 vs 191.6 ms/step without, so
  // the default leaves the latency to the other wave
  if (v == AV_GT_PREFETCH) return plan_analysis_mfma_g_kernel(np, fd, OBS_DN16, true, false, SPEC_ANY);
  const bool prop = a.prop && !a.reg_v;   // fused forecast, no regulariser
  if (np == 10 && v == AV_MIXLO_SPLIT)
    return plan_analysis_mfma_g_mixlo_kernel(np, fd, OBS_DN16, false, true, prop ? SPEC_PROP : SPEC_ANY);
  // the launch's paths fixed at compile time (SPEC_PROP)
  if (prop && v == AV_DEFAULT && il0) return plan_analysis_mfma_g_kernel(np, fd, OBS_DN16, false, true, SPEC_PROP);
  return plan_analysis_mfma_g_kernel(np, fd, OBS_DN16, false, il0 != (v == AV_BLOCK_ORDER), SPEC_ANY);
}

// The kernel of an analysis launch.  Fast-path instantiations: JRC-TIP (7
// params, 4-input band GPs), PROSAIL (10 params, full-state GPs), full-state
// GPs for small states, and all-precomputed / all-linear operators.
inline KernelPlan analysis_plan(int np, const AnalysisArgs& a) {
  if (!plan_np(np)) return KernelPlan{};
  const int fd = a.fast_d, obs = a.fast_obs, v = a.variant;
  const bool f32dn = obs == OBS_DN16 || obs == OBS_F32;
  KernelPlan p = plan_analysis_kernel(np, 0, 0);
  if (fd == FD_PRECOMP || fd == FD_LINEAR) {
    // bf16 (y, w) observations: precomputed / linear operators only
    if (f32dn || obs == OBS_BF16 || obs == OBS_BF16Y) p = plan_analysis_kernel(np, fd, obs);
  } else if (f32dn && (np == 7 ? fd == 4 || fd == 7 : fd == np)) {
    // GP on the matrix cores when the host attached split-f16 tables to every band
    // (AV_VALU_ORACLE: the f32 VALU record loop, the tests' second device path)
    const bool mc = fd <= GPM_MAX_D && v != AV_VALU_ORACLE;
    if (mc && a.gpm_frags > 0 && a.n_bands <= GPM_MAX_BANDS) p = analysis_plan_lds(np, a);
    else if (mc && fd == np && np >= 7 && a.gpm_global) p = analysis_plan_global(np, a);
    else p = plan_analysis_kernel(np, fd, obs);
  }
  // AV_MIXLO_SPLIT (gpm_exp_split's MIXLO flag: the split of m before
  // profiles/split_issue_probe.jsonl) is instantiated for the kernels its test
  // and its A/B run, DN16 observations only: the JRC-TIP LDS-table kernel and
  // the 10-parameter global-table kernel, in both analysis forms.  Any other
  // launch with it is an error, not another kernel.
  if (v == AV_MIXLO_SPLIT && !p.mixlo) return KernelPlan{};
  return p;
}

// The kernel of a gain launch: the all-GP fast instantiations (as
// analysis_plan) or the generic kernel.  The host selects the VALU oracle by
// attaching no tables (ops/kernels.py gain: gpm_frags = 0, gpm_global = 0).
inline KernelPlan gain_plan(int np, const GainArgs& a) {
  if (!plan_np(np)) return KernelPlan{};
  const int fd = a.fast_d, obs = a.fast_obs;
  const bool gp = obs == OBS_DN16 || obs == OBS_F32;
  const bool mixlo = obs == OBS_DN16 && a.split_mixlo;
  KernelPlan p = plan_gain_kernel(np, 0, 0);
  if (gp && np == 7 && fd == 4) {
    // JRC-TIP: tables staged in LDS
    if (a.gpm_frags > 0 && a.n_bands <= GPM_MAX_BANDS)
      p = mixlo ? plan_gain_mfma_mixlo_kernel(np, fd, obs) : plan_gain_mfma_kernel(np, fd, obs);
    else p = plan_gain_kernel(np, fd, obs);
  } else if (gp && np == 10 && fd == 10) {
    // full-state GP bands with global tables
    if (a.gpm_global) p = mixlo ? plan_gain_mfma_g_mixlo_kernel(np, fd, obs) : plan_gain_mfma_g_kernel(np, fd, obs);
    else p = plan_gain_kernel(np, fd, obs);
  }
  if (a.split_mixlo && !p.mixlo) return KernelPlan{};   // as AV_MIXLO_SPLIT in analysis_plan
  return p;
}

}  // namespace kf
