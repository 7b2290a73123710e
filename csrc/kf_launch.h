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
hipError_t dev_gp_operator(int np, int d, const GpOperatorArgs& a, hipStream_t s);
bool gp_operator_supported(int np, int d);
hipError_t dev_unpack(int np, const RasterArgs& a, hipStream_t s);
hipError_t dev_marginal(int np, const RasterArgs& a, hipStream_t s);       // a.kind: MARG_*
hipError_t dev_product(int np, const ProductArgs& a, hipStream_t s);       // physical-unit planes, interval, QA byte
hipError_t dev_smooth(int np, const SmoothArgs& a, hipStream_t s);         // one backward step of the RTS smoother
hipError_t dev_innovation(int np, const InnovationArgs& a, hipStream_t s); // statistics and the chi-square gate
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
