// kf_launch.h — launcher entry points (device: kf_kernels.hip + kf_analysis{7,10}.hip,
// host: kf_host.cpp).
#pragma once
#include <stdint.h>
#include <vector>
#include "kf_core.h"
#include "kf_plan.h"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#else
#include <hip/hip_runtime_api.h>
#endif

// Grid cap for the grid-stride kernels (A/B, scripts/gpu_grid.sh: 16384 is 3 %
// faster than 4096 at 15M and 120M px; round 4, scripts/gpu_r4_v22.sh at 120M
// px: 768 persistent blocks 45.6 ms, 16384 42.2, 32768-131072 41.9, one pixel
// per thread 42.8 -- the cloud skip makes blocks uneven, so more blocks finish
// closer together, up to the point where the per-block LDS table staging and
// dispatch cost more).
#define KF_MAX_BLOCKS 65536

namespace kf {

int dev_grid(int64_t N);
void set_max_blocks(int n);
void set_gp_unroll(int n);
int get_max_blocks();
// *n_part: norm partial entries written (workgroups of the grid-stride launch)
hipError_t dev_analysis(int np, const AnalysisArgs& a, int grid, hipStream_t s, int* n_part);
hipError_t dev_analysis_np7(const AnalysisArgs& a, int grid, hipStream_t s);
hipError_t dev_analysis_np10(const AnalysisArgs& a, int grid, hipStream_t s);
#ifdef KF_PHASE_CLOCKS
hipError_t phase_clocks_np7(unsigned long long* out, bool reset);
hipError_t phase_clocks_np10(unsigned long long* out, bool reset);
#endif
hipError_t dev_gain(int np, const GainArgs& a, int grid, hipStream_t s);
hipError_t dev_gain_np10(const GainArgs& a, int grid, hipStream_t s);
// the plan of every line of the K1 / K1g launch tables (kf_device.h KF_ROW), all translation units
std::vector<KernelPlan> dev_launch_table();
void launch_table_np7(std::vector<KernelPlan>& out);
void launch_table_np10(std::vector<KernelPlan>& out);
void launch_table_gain_np10(std::vector<KernelPlan>& out);
hipError_t dev_jacobi(int np, const JacobiArgs& a, int grid, hipStream_t s);
// The auxiliary per-pixel passes (kf_core.h KF_PIXEL_OP): one pixel_kernel launch over a.N pixels each,
// the grid capped by set_max_blocks
hipError_t dev_propagate(int np, const PropArgs& a, hipStream_t s);
hipError_t dev_invert(int np, const InvertArgs& a, hipStream_t s);
hipError_t dev_operator(int np, const OperatorArgs& a, hipStream_t s);
hipError_t dev_hessian(int np, const HessianArgs& a, hipStream_t s);
// K6 on the matrix cores (kf_hessian_mfma.hip): hessian_plan's PLAN_HESSIAN_MFMA kernel for a
hipError_t dev_hessian_mfma(const KernelPlan& plan, const HessianMfmaArgs& a, hipStream_t s);
void launch_table_hessian(std::vector<KernelPlan>& out);
// GP predictive variance on the matrix cores (kf_gp_variance.hip): out[p] = s (1 - |W^ k^(x_p)|^2) for one
// emulator, with K + nugget = L L^T, k^ = k / s and W^ = sqrt(s) L^-1 (tables: models/gp.py
// mfma_variance_tables).  The GP input d of pixel p is x[map[d] * ld + p] - center[d].
constexpr int GPV_MAX_CHUNKS = 16;   // 32-point chunks: k^ of a 64-pixel tile in LDS, 8 KiB per chunk
struct GpVarArgs {
  const float* x;     // SoA state rows [n_params][ld] (read only)
  float* out;         // [N]
  int64_t N, ld;
  const void* etab;   // exponent A fragments, nchunk x gpm_k_steps(d) x 64 x 16 B
  const void* wtab;   // W^ hi / lo A fragments, nchunk (nchunk + 1) / 2 blocks x 4 KiB
  int32_t nchunk, d;
  float signal;       // s
  float inv_scale2;   // 1 / w_scale^2: undoes the power-of-two scale of W^ on sum u^2
  int32_t map[GPM_MAX_D];
  float center[GPM_MAX_D];
  float lam[GPM_MAX_D];
};
// grid <= 0: one workgroup per compute unit (the kernel keeps a CU's LDS to itself)
hipError_t dev_gp_variance(const GpVarArgs& a, int grid, hipStream_t s);
std::vector<const char*> gp_variance_table();
// the same whitened form as a float32 loop: t [T][d] centred training inputs, w [T][T] the unsplit W^
int host_gp_variance(const GpVarArgs& a, const float* t, const float* w, int T);
// Observation error inflated by the emulator's predictive variance (kf_gp_variance.hip gp_obs_weight_kernel):
// for every band b of the launch and pixel p, with (y, w) = decode_obs(band, p) and var = the band's
// predictive variance at x_p, y_out[p] = y and w_out[p] = w / (1 + w var) = 1 / (sigma_obs^2 + var) -- the
// (y, w) planes of an OBS_F32 band -- and var_out[p] = var (may be null).  A 64-pixel tile without an
// observation reads (y, 0, var 0) and costs no GP work; a pixel whose GP input is not finite keeps its w.
constexpr int GPW_MAX_BANDS = 8;   // bands per launch (the caller slices longer tables)
struct GpObsWeightBand {
  const void* etab;   // GpVarArgs' table fields
  const void* wtab;
  int32_t nchunk, d;
  float signal, inv_scale2;
  int32_t map[GPM_MAX_D];
  float center[GPM_MAX_D];
  float lam[GPM_MAX_D];
  int32_t obs;        // what decode_obs reads of a BandDesc
  float scale, rel_unc, unc_floor;
  const float* y;
  const float* w;
  const uint8_t* mask;
  const uint16_t* dn;
  float* y_out;       // [N]
  float* w_out;       // [N]
  float* var_out;     // [N] or null
};
struct GpObsWeightArgs {
  const float* x;     // SoA state rows [n_params][ld] (read only)
  int64_t N, ld;
  int32_t nb, pad0;
  GpObsWeightBand band[GPW_MAX_BANDS];
};
// B: GpObsWeightBand, in the kernel behind the kernarg pointer
template <typename B>
KF_HD void gpw_decode(const B& b, int64_t p, float& y, float& w) {
  BandDesc bd{};   // decode_obs' fields only; the rest folds away
  bd.obs = b.obs;
  bd.scale = b.scale;
  bd.rel_unc = b.rel_unc;
  bd.unc_floor = b.unc_floor;
  bd.y = b.y;
  bd.w = b.w;
  bd.mask = b.mask;
  bd.dn = b.dn;
  decode_obs<0>(bd, p, y, w);
}
// the inflated weight: a true division (w var is no small term where the emulator extrapolates); w = 0 stays
// +0, and a variance that could not be evaluated (fin false) leaves w as decoded
KF_HD float gpw_weight(float w, float var, bool fin) { return fin ? w / __builtin_fmaf(w, var, 1.f) : w; }
// grid <= 0: one workgroup per compute unit and band.  One launch per distinct d of the bands.
hipError_t dev_gp_obs_weight(const GpObsWeightArgs& a, int grid, hipStream_t s);
// t[b] [T[b]][d] centred training inputs, w[b] [T[b]][T[b]] the unsplit W^ of band b
int host_gp_obs_weight(const GpObsWeightArgs& a, const float* const* t, const float* const* w, const int* T);
hipError_t dev_gp_operator(int np, int d, const GpOperatorArgs& a, hipStream_t s);
bool gp_operator_supported(int np, int d);
// K2 on the matrix cores (kf_gp_operator_mfma.hip): one grid per plan of gp_operator_plan (a distinct input
// count each) over a's bands, a.g.nb <= GPO_MAX_BANDS; max_blocks caps the workgroups of a launch
hipError_t dev_gp_operator_mfma(const std::vector<KernelPlan>& plans, const GpOperatorMfmaArgs& a, hipStream_t s);
void launch_table_gp_operator(std::vector<KernelPlan>& out);
// K2 in float64 (kf_gp_operator_f64.hip): one grid per plan of gp_operator_f64_plan (a distinct NK each)
hipError_t dev_gp_operator_f64(const std::vector<KernelPlan>& plans, const GpOperatorF64Args& a, hipStream_t s);
void launch_table_gp_operator_f64(std::vector<KernelPlan>& out);
hipError_t dev_unpack(int np, const RasterArgs& a, hipStream_t s);
hipError_t dev_marginal(int np, const RasterArgs& a, hipStream_t s);       // a.kind: MARG_*
hipError_t dev_product(int np, const ProductArgs& a, hipStream_t s);       // physical-unit planes, interval, QA byte
hipError_t dev_smooth(int np, const SmoothArgs& a, hipStream_t s);         // one backward step of the RTS smoother
hipError_t dev_smooth_r1(int np, const SmoothR1Args& a, hipStream_t s);    // ... for one propagated parameter
// statistics and the chi-square gate; plan: innovation_plan's kernel for a (kf_plan.h), the VALU pixel_kernel
// or one of the matrix-core kernels of kf_innovation_mfma.hip
hipError_t dev_innovation(int np, const InnovationArgs& a, const KernelPlan& plan, hipStream_t s);
hipError_t dev_innovation_mfma(const KernelPlan& plan, const InnovationArgs& a, int grid, hipStream_t s);
void launch_table_innovation(std::vector<KernelPlan>& out);
// ... at the fused forecast (a.prop set): the kernels of KF_INNOV_PROP_ROWS, a table of their own
hipError_t dev_innovation_prop(const KernelPlan& plan, const InnovationArgs& a, int grid, hipStream_t s);
void launch_table_innovation_prop(std::vector<KernelPlan>& out);
hipError_t dev_reduce(const double* partials, int n, double* out, hipStream_t s);
hipError_t dev_gather(int elem_bytes, const void* src, const int64_t* idx, void* dst, int64_t n, int rows,
                      int64_t src_ld, int64_t dst_ld, hipStream_t s);
hipError_t dev_lut_nearest(const float* lut, int M, int D, const float* x, int64_t N, int64_t ld, int32_t* out,
                           hipStream_t s);
// test kernel: the f16 bit patterns of gpm_exp_split's hi / lo halves of m[i] = 2^e[i],
// n8 groups of 8 values, 16-byte aligned (mixlo: the AV_MIXLO_SPLIT body)
hipError_t dev_exp_split_probe(const float* e, uint16_t* mh, uint16_t* ml, float* m, int64_t n8, bool mixlo,
                               hipStream_t s);
hipError_t dev_reg_tiled(const RegTileArgs& a, hipStream_t s);
int reg_rho_blocks(int64_t N);
hipError_t dev_reg_rho(const float* vrow, const StripGeo& g, int64_t N, const RegScheduleArgs& a, hipStream_t s);
hipError_t dev_reg_schedule(const RegScheduleArgs& a, hipStream_t s);

// per-chunk Gauss-Newton convergence (kf_core.h ChunkPartialArgs ...)
constexpr int KF_CMP_CHUNK = 4096;   // visiting slots per compaction workgroup
int chunk_compact_blocks(int64_t n);
hipError_t dev_chunk_partials(const ChunkPartialArgs& a, hipStream_t s);
hipError_t dev_chunk_decide(const ChunkDecideArgs& a, hipStream_t s);
hipError_t dev_chunk_compact(const ChunkCompactArgs& a, hipStream_t s);
int host_chunk_partials(const ChunkPartialArgs& a);
int host_chunk_decide(const ChunkDecideArgs& a);
int64_t host_chunk_compact(const ChunkCompactArgs& a);

// Host runner: the same per-pixel code over OpenMP; the block partition
// mirrors the device grid-stride mapping so partials have the same meaning.
inline bool host_supported(int np) { return plan_np(np); }
int host_analysis(int np, const AnalysisArgs& a, int grid);
int host_gain(int np, const GainArgs& a, int grid);
int host_jacobi(int np, const JacobiArgs& a, int grid);
int host_propagate(int np, const PropArgs& a);
int host_invert(int np, const InvertArgs& a);
int host_operator(int np, const OperatorArgs& a);
int host_hessian(int np, const HessianArgs& a);
int host_gp_operator(int np, const GpOperatorArgs& a);
int host_unpack(int np, const RasterArgs& a);
int host_marginal(int np, const RasterArgs& a);
int host_product(int np, const ProductArgs& a);
int host_smooth(int np, const SmoothArgs& a);
int host_smooth_r1(int np, const SmoothR1Args& a);
int host_innovation(int np, const InnovationArgs& a);
// obs_order chunk: pixels per scatter workgroup; local = 1 partitions each
// chunk on its own (no count / scan passes, chunk-aligned, see kf_kernels.hip)
constexpr int KF_ORD_CHUNK = 4096;
int obs_order_chunks(int64_t N);
hipError_t dev_obs_order(const BandDesc* bands, const int32_t* grp, int nb, int G, int64_t N, int32_t* counts,
                         int32_t* order, bool local, hipStream_t s);
int host_obs_order(const BandDesc* bands, const int32_t* grp, int nb, int G, int64_t N, int32_t* order, bool local);
int host_lut_nearest(const float* lut, int M, int D, const float* x, int64_t N, int64_t ld, int32_t* out);
int host_reg_tiled(const RegTileArgs& a);
int host_reg_rho(const float* vrow, const StripGeo& g, int64_t N, const RegScheduleArgs& a);
int host_reg_schedule(const RegScheduleArgs& a);

// GeoTIFF tile encoder (kf_deflate.h / kf_deflate.hip): planes [nplanes][plane_ld]
// of H x W float32 rasters -> one zlib stream per 256 x 256 tile at
// out + tile * DFL_BOUND, its byte count in sizes[tile] (tiles plane-major,
// row-major within a plane)
struct DflArgs {
  const float* src;
  int64_t plane_ld;
  int32_t H, W, nplanes, tiles_x, tiles_y, mode;   // mode: DFL_MODE_* (kf_deflate.h); 0 = fixed Huffman
  uint8_t* out;
  uint32_t* sizes;
  uint8_t* scratch;   // device: DFL_TILE * DFL_ROW_WORDS words per tile (row bit strings before the shift;
                      // DFL_ROW_WORDS_DYN in the dynamic mode)
  // fmt: DFL_FMT_* (kf_deflate.h); 0 = float32 samples under predictor 3, the
  // fields below unused.  DFL_FMT_U16: the planes are quantised to scaled 16-bit
  // samples in the row load (q = clamp(rint(fma(v, qa[plane], qb[plane])), 0,
  // 65534), NaN -> 65535) and written under predictor 2; tiles then lie at
  // out + tile * DFL_BOUND16, the row scratch is DFL_ROW_WORDS16(_DYN) words per
  // row, and sat[plane] (may be null) is incremented by the plane's samples
  // whose rounded value fell outside [0, 65534]
  int32_t fmt;
  const float* qa;
  const float* qb;
  uint32_t* sat;
};
hipError_t dev_deflate_tiles(const DflArgs& a, hipStream_t s);
// bound: the tiles' stride in scratch (DFL_BOUND, or DFL_BOUND16 for 16-bit tiles)
hipError_t dev_deflate_pack(const uint8_t* scratch, const uint32_t* sizes, const int64_t* offs, uint8_t* packed,
                            int ntiles, hipStream_t s, int64_t bound);
int host_deflate_tiles(const DflArgs& a);
// the planes' samples quantised as the DFL_FMT_U16 encoder quantises them
// (dfl_quantise): dst [nplanes][H * W] uint16, sat[plane] += saturated samples
int host_quantise_u16(const float* src, int64_t plane_ld, int64_t n, int nplanes, const float* qa, const float* qb,
                      uint16_t* dst, uint32_t* sat);

// GeoTIFF tile decoder (kf_inflate.h / kf_inflate.hip): one status per tile
constexpr int32_t INF_OK = 0;
constexpr int32_t INF_TRUNCATED = 1;      // the stream (or its byte range in `comp`) ends too early
constexpr int32_t INF_BAD_HEADER = 2;     // zlib header: CM, CINFO, FCHECK or FDICT
constexpr int32_t INF_BAD_BLOCK = 3;      // BTYPE 11
constexpr int32_t INF_BAD_STORED = 4;     // LEN / NLEN mismatch
constexpr int32_t INF_BAD_CODE = 5;       // a dynamic block's code lengths describe no usable code
constexpr int32_t INF_BAD_SYMBOL = 6;     // bits that are no code, or a reserved symbol
constexpr int32_t INF_BAD_DISTANCE = 7;   // a match reaches before the tile's first byte
constexpr int32_t INF_OVERRUN = 8;        // more output than the raw size
constexpr int32_t INF_SHORT = 9;          // end of stream before the raw size
constexpr int32_t INF_BAD_ADLER = 10;
constexpr int32_t INF_NSTATUS = 11;

// Tiles i < ntiles: the zlib stream comp[offs[i], offs[i] + sizes[i]) inflates
// to raw_bytes bytes = a tile x tile block of elem_bytes samples at tile row /
// column tile_rc[2 i], tile_rc[2 i + 1] of a raster; the TIFF predictor is
// undone per tile row and the tile's intersection with the window rows
// [r0, r1) x columns [c0, c1) is written to dst (row-major, ld elements per
// row, element (r0, c0) first).  status[i] = INF_*; a tile that fails leaves
// its part of the window zeroed.  The window must lie inside the raster, so a
// padded edge tile's padding is never written.
struct InfArgs {
  const uint8_t* comp;
  int64_t comp_bytes;
  const int64_t* offs;
  const int64_t* sizes;
  const int32_t* tile_rc;
  int32_t ntiles, tile, elem_bytes, predictor;   // tile: 256; 2 bytes: predictor 1 / 2; 4 bytes: 1 / 3
  int64_t raw_bytes;
  int64_t r0, r1, c0, c1;
  void* dst;
  int64_t ld;
  int32_t* status;
  uint8_t* scratch;   // device: ntiles * inf_scratch_stride(raw_bytes, tile, elem_bytes) bytes, 16-byte aligned
};
hipError_t dev_inflate_tiles(const InfArgs& a, hipStream_t s);
int host_inflate_tiles(const InfArgs& a);
int64_t host_inflate_count_tokens(const uint8_t* comp, int64_t comp_bytes, const int64_t* offs, const int64_t* sizes,
                                  int ntiles, int64_t raw_bytes);

}  // namespace kf
