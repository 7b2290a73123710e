// kf_host.cpp — CPU runner for the per-pixel kernels of kf_core.h.
// Compiled by g++ (-fopenmp); the math is byte-for-byte the source the
// gfx950 kernels run, so CPU CI exercises the kernel code paths.
#include <omp.h>
#include <math.h>
#include <string.h>
#include "kf_launch.h"
#include "kf_deflate.h"
#include "kf_inflate.h"
#include <algorithm>
#include <vector>

namespace kf {

static constexpr int HBLOCK = 256;

// Block b handles pixels p = b*256 + t + k*grid*256 (same as the device).
template <typename F>
static void grid_stride(int64_t N, int grid, double* partials, F&& f) {
  const int64_t stride = (int64_t)grid * HBLOCK;
#pragma omp parallel for schedule(dynamic, 4)
  for (int b = 0; b < grid; ++b) {
    double acc = 0.0;
    for (int t = 0; t < HBLOCK; ++t)
      for (int64_t p = (int64_t)b * HBLOCK + t; p < N; p += stride) acc += (double)f(p);
    if (partials) partials[b] = acc;
  }
}

// The same mapping over the visiting slots q of a K1 / K1g launch (pixel
// order[q], visit_count slots), with both norm accumulators of a fused
// two-iteration launch: f(p, dn1) -> dn.
template <typename A, typename F>
static void grid_stride_visit(const A& a, int grid, F&& f) {
  const int64_t stride = (int64_t)grid * HBLOCK;
  const int64_t nv = visit_count(a);
#pragma omp parallel for schedule(dynamic, 4)
  for (int b = 0; b < grid; ++b) {
    double acc = 0.0, acc1 = 0.0;
    for (int t = 0; t < HBLOCK; ++t)
      for (int64_t q = (int64_t)b * HBLOCK + t; q < nv; q += stride) {
        float dn1;
        acc += (double)f(visit_px(a.order, q), dn1);
        acc1 += (double)dn1;
      }
    if (a.partials) a.partials[b] = acc;
    if (a.partials_first) a.partials_first[b] = acc1;
  }
}

template <int NP>
static void h_analysis(const AnalysisArgs& a, int grid) {
  // JRC-TIP structure of the fused forecast's precision (AnalysisArgs.a_struct,
  // checked by the caller): the structure-aware solve, as the SPEC_*_TIP kernels
  const bool tip = NP == 7 && (a.a_struct & A_STRUCT_TIP) && a.prop && a.variant != AV_DENSE_SOLVE;
  grid_stride_visit(a, grid, [&](int64_t p, float& dn1) {
    float dn;
    if constexpr (NP == 7) {
      dn = tip ? pixel_analysis<NP, 0, 0, 4, false, StructTip>(a, p, dn1) : pixel_analysis<NP>(a, p, dn1);
    } else {
      dn = pixel_analysis<NP>(a, p, dn1);
    }
    if (a.dn_out) a.dn_out[p] = dn;
    return dn;
  });
}

// Every auxiliary per-pixel pass (kf_core.h KF_PIXEL_OP), as pixel_kernel runs it
// on the device: OP::px<NP>(a, p) for every p < a.N; -1 for a state size with
// no compiled code.
template <class OP>
static int host_pixels(int np, const typename OP::Args& a) {
  const bool known = np_dispatch(np, [&](auto n) {
#pragma omp parallel for schedule(static)
    for (int64_t p = 0; p < a.N; ++p) OP::template px<decltype(n)::value>(a, p);
  });
  return known ? 0 : -1;
}

// K2 split path on the host: any band operator, any input count
struct OpGpOperatorHost {
  using Args = GpOperatorArgs;
  template <int NP>
  static void px(const Args& a, int64_t p) {
    pixel_gp_operator<NP>(a, p, [&](const BandDesc& bd, int, const float (&xv)[NP], float& H0, float (&hv)[NP]) {
      eval_operator<NP>(bd, p, a.ld, xv, H0, hv);
    });
  }
};

// GeoTIFF tiles on the host: the same row encoder as dfl_tile_kernel, rows in
// order into one byte stream per tile (bit-identical streams).  Dynamic mode:
// the same two passes as dfl_tile_dyn_kernel (histogram, table, encode).
// FMT = DFL_FMT_U16: the row's samples quantised (dfl_quantise) and differenced
// as 16-bit words in the row functor, as the kernel's row load does.
// Returns -2 if a tile's stream is not the size its table announced.
template <int FMT>
static int host_deflate_tiles_fmt(const DflArgs& a) {
  const int per = a.tiles_x * a.tiles_y, n = a.nplanes * per;
  constexpr int64_t BOUND = dfl_bound(FMT), RAW = dfl_raw(FMT);
  constexpr int ROW = dfl_row_len(FMT);
  int bad = 0;
  std::vector<uint32_t> satv((size_t)a.nplanes, 0u);
  uint32_t* satp = satv.data();
#pragma omp parallel for schedule(dynamic, 1) reduction(| : bad)
  for (int tile = 0; tile < n; ++tile) {
    const int plane = tile / per, tt = tile - plane * per;
    const int ty = tt / a.tiles_x, tx = tt - ty * a.tiles_x;
    const int x0 = tx * DFL_TILE;
    const int ncol = a.W - x0 < DFL_TILE ? a.W - x0 : DFL_TILE;
    uint8_t* o = a.out + (int64_t)tile * BOUND;
    int64_t nb = 0;
    uint64_t acc = 0;
    int nacc = 0;
    auto sink = [&](uint32_t bits, int len) {
      acc |= (uint64_t)bits << nacc;
      nacc += len;
      while (nacc >= 8) {
        o[nb++] = (uint8_t)(acc & 0xFFu);
        acc >>= 8;
        nacc -= 8;
      }
    };
    const float qa = FMT == DFL_FMT_U16 ? a.qa[plane] : 0.f, qb = FMT == DFL_FMT_U16 ? a.qb[plane] : 0.f;
    uint32_t sat = 0;
    // fn(row, rest) for every row of the tile
    auto rows = [&](auto&& fn) {
      for (int r = 0; r < DFL_TILE; ++r) {
        const int64_t y = (int64_t)ty * DFL_TILE + r;
        const bool rin = y < a.H;
        const float* rowp = a.src + (int64_t)plane * a.plane_ld + (rin ? y : 0) * a.W + x0;
        if constexpr (FMT == DFL_FMT_U16) {
          uint32_t qprev = 0, d = 0;
          auto row = [&](int i) -> uint32_t {     // byte i of the row's 16-bit differences, i ascending
            if (!(i & 1)) {
              const int c = i >> 1;
              const uint32_t q = (rin && c < ncol) ? dfl_quantise(rowp[c], qa, qb, sat) : 0u;
              d = (q - (c ? qprev : 0u)) & 0xFFFFu;
              qprev = q;
            }
            return (d >> (8 * (i & 1))) & 0xFFu;
          };
          fn(row, RAW - (int64_t)r * ROW);
        } else {
          auto row = [&](int c) -> uint32_t {
            if (!(rin && c < ncol)) return 0u;
            uint32_t u;
            memcpy(&u, rowp + c, 4);
            return u;
          };
          fn(row, RAW - (int64_t)r * ROW);
        }
      }
    };
    sink(0x78u, 8);
    sink(0x01u, 8);
    uint64_t t1 = 0, t2 = 0;
    if (a.mode == DFL_MODE_FIXED) {
      sink(1u, 1);                 // BFINAL
      sink(1u, 2);                 // BTYPE 01: fixed Huffman
      rows([&](auto& row, int64_t rest) {
        uint64_t s1, s2;
        dfl_encode_row<FMT>(row, rest, sink, s1, s2);
        t1 += s1;
        t2 += s2;
      });
      sink(0u, 7);                 // end of block
    } else {
      uint32_t freq[DFL_NSYM] = {0};
      DflTable t;
      DflWork k;
      rows([&](auto& row, int64_t rest) {
        uint64_t s1, s2;
        dfl_tokenise_row<FMT>(row, rest, [&](uint32_t v, int L) { ++freq[dfl_token_symbol(v, L)]; }, s1, s2);
        t1 += s1;
        t2 += s2;
      });
      const uint32_t sat1 = sat;   // the second pass quantises the same samples again
      freq[256] = 1;
      int used = 0;
      for (int s = 0; s < DFL_NSYM; ++s) {
        const int rk = dfl_rank(freq, DFL_NSYM, s);
        if (rk >= 0) {
          k.sorted[rk] = (uint16_t)s;
          ++used;
        }
      }
      dfl_choose_table(freq, used, a.mode == DFL_MODE_DYNAMIC_FORCE_FIXED, t, k);
      dfl_write_block_header(t, sink);
      if ((uint64_t)(nb - 2) * 8 + (uint64_t)nacc != t.head_bits) bad |= 1;
      rows([&](auto& row, int64_t rest) {
        uint64_t s1, s2;
        dfl_tokenise_row<FMT>(row, rest, [&](uint32_t v, int L) {
          uint32_t b;
          int l;
          dfl_table_token(t, v, L, b, l);
          sink(b, l);
        }, s1, s2);
      });
      sat = sat1;
      sink(t.code[256], t.len[256]);   // end of block
      if ((uint64_t)(nb - 2) * 8 + (uint64_t)nacc != t.block_bits) bad |= 1;
    }
    if (nacc) sink(0u, 8 - nacc);
    const uint32_t adler = dfl_adler(t1, t2, RAW);
    for (int k = 3; k >= 0; --k) sink((adler >> (8 * k)) & 0xFFu, 8);
    a.sizes[tile] = (uint32_t)nb;
    if (FMT == DFL_FMT_U16 && sat) {
#pragma omp atomic
      satp[plane] += sat;
    }
  }
  if (FMT == DFL_FMT_U16 && a.sat)
    for (int p = 0; p < a.nplanes; ++p) a.sat[p] += satv[(size_t)p];
  return bad ? -2 : 0;
}

int host_deflate_tiles(const DflArgs& a) {
  if (a.nplanes * a.tiles_x * a.tiles_y <= 0) return -1;
  if (a.mode != DFL_MODE_FIXED && a.mode != DFL_MODE_DYNAMIC && a.mode != DFL_MODE_DYNAMIC_FORCE_FIXED) return -1;
  if (a.fmt == DFL_FMT_F32) return host_deflate_tiles_fmt<DFL_FMT_F32>(a);
  if (a.fmt == DFL_FMT_U16 && a.qa && a.qb) return host_deflate_tiles_fmt<DFL_FMT_U16>(a);
  return -1;
}

int host_quantise_u16(const float* src, int64_t plane_ld, int64_t n, int nplanes, const float* qa, const float* qb,
                      uint16_t* dst, uint32_t* sat) {
  if (n < 0 || nplanes <= 0 || !qa || !qb) return -1;
  for (int p = 0; p < nplanes; ++p) {
    const float* s = src + (int64_t)p * plane_ld;
    uint16_t* d = dst + (int64_t)p * n;
    const float a = qa[p], b = qb[p];
    uint64_t total = 0;
#pragma omp parallel for schedule(static) reduction(+ : total)
    for (int64_t i = 0; i < n; ++i) {
      uint32_t one = 0;
      d[i] = (uint16_t)dfl_quantise(s[i], a, b, one);
      total += one;
    }
    if (sat) sat[p] += (uint32_t)total;
  }
  return 0;
}

// GeoTIFF tiles inflated on the host: the decoder of inf_tile_kernel
// (kf_inflate.h: inf_step) with the serial drain, one tile per OpenMP
// iteration, then the predictor undo and the placement into the window.
int host_inflate_tiles(const InfArgs& a) {
  if (!inf_args_ok(a)) return -1;
  const int T = a.tile, e = a.elem_bytes;
  const int64_t row_bytes = (int64_t)T * e, tile_bytes = row_bytes * T;
  const int64_t stride = inf_scratch_stride(a.raw_bytes, T, e);
  const uint32_t n = (uint32_t)a.raw_bytes;
#pragma omp parallel
  {
    std::vector<uint8_t> raw((size_t)stride), tmp((size_t)row_bytes);
    InfTables tab;
    uint32_t q[INF_QUEUE];
#pragma omp for schedule(dynamic, 1)
    for (int tile = 0; tile < a.ntiles; ++tile) {
      const int64_t off = a.offs[tile], sz = a.sizes[tile];
      int32_t status = INF_OK;
      if (off < 0 || sz < 0 || sz > 0x7FFFFFFF || off > a.comp_bytes || sz > a.comp_bytes - off) {
        status = INF_TRUNCATED;         // the byte range is not inside comp
      } else {
        InfState st;
        inf_init(st, a.comp + off, (uint32_t)sz, n);
        uint32_t pos = 0;
        uint64_t s1 = 0, s2 = 0;
        for (;;) {
          const int nq = inf_step(st, tab, q, INF_QUEUE);
          inf_drain_serial(q, nq, raw.data(), pos, n, s1, s2);
          for (uint32_t j = 0; j < st.sto_len; ++j) {
            KF_DCHECK(pos + j < n && st.sto_off + j < st.n);
            const uint32_t b = st.in[st.sto_off + j];
            raw[pos + j] = (uint8_t)b;
            inf_adler_add(s1, s2, b, pos + j, n);
          }
          pos += st.sto_len;
          if (st.status != INF_OK || st.phase == INF_P_DONE) break;
        }
        status = st.status;
        if (status == INF_OK && dfl_adler(s1, s2, (int64_t)n) != st.adler) status = INF_BAD_ADLER;
        for (int64_t i = a.raw_bytes; i < tile_bytes; ++i) raw[(size_t)i] = 0;   // a raw size short of a tile
      }
      a.status[tile] = status;
      // the tile's part of the window
      const int64_t gy0 = (int64_t)a.tile_rc[2 * tile] * T, gx0 = (int64_t)a.tile_rc[2 * tile + 1] * T;
      const int64_t ya = std::max(gy0, a.r0), yb = std::min(gy0 + T, a.r1);
      const int64_t xa = std::max(gx0, a.c0), xb = std::min(gx0 + T, a.c1);
      if (ya >= yb || xa >= xb) continue;
      uint8_t* dst = static_cast<uint8_t*>(a.dst);
      for (int64_t y = ya; y < yb; ++y) {
        uint8_t* d = dst + ((y - a.r0) * a.ld + (xa - a.c0)) * e;
        KF_DCHECK(y - a.r0 < a.r1 - a.r0 && xb - a.c0 <= a.ld);
        if (status != INF_OK) {
          memset(d, 0, (size_t)((xb - xa) * e));
          continue;
        }
        uint8_t* row = raw.data() + (y - gy0) * row_bytes;
        KF_DCHECK((y - gy0 + 1) * row_bytes <= stride);
        if (a.predictor == 2) {         // 16-bit horizontal differencing
          uint16_t acc = 0;
          for (int c = 0; c < T; ++c) {
            uint16_t v;
            memcpy(&v, row + 2 * c, 2);
            acc = (uint16_t)(acc + v);
            memcpy(row + 2 * c, &acc, 2);
          }
        } else if (a.predictor == 3) {  // float32: byte differences of the 4 byte planes, most significant first
          uint8_t acc = 0;
          for (int64_t i = 0; i < row_bytes; ++i) {
            acc = (uint8_t)(acc + row[i]);
            tmp[(size_t)i] = acc;
          }
          for (int c = 0; c < T; ++c)
            for (int b = 0; b < 4; ++b) row[4 * c + b] = tmp[(size_t)((3 - b) * T + c)];
        }
        memcpy(d, row + (xa - gx0) * e, (size_t)((xb - xa) * e));
      }
    }
  }
  return 0;
}

// Literal + match tokens of the streams (nothing is written): what the
// decoder lane of inf_tile_kernel processes, for a symbols-per-second figure.
// -1 if a stream does not decode to raw_bytes.
int64_t host_inflate_count_tokens(const uint8_t* comp, int64_t comp_bytes, const int64_t* offs, const int64_t* sizes,
                                  int ntiles, int64_t raw_bytes) {
  int64_t total = 0;
  bool bad = false;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : total) reduction(|| : bad)
  for (int tile = 0; tile < ntiles; ++tile) {
    if (offs[tile] < 0 || sizes[tile] < 0 || sizes[tile] > 0x7FFFFFFF || offs[tile] > comp_bytes ||
        sizes[tile] > comp_bytes - offs[tile]) {
      bad = true;
      continue;
    }
    InfTables tab;
    InfState st;
    uint32_t q[INF_QUEUE];
    inf_init(st, comp + offs[tile], (uint32_t)sizes[tile], (uint32_t)raw_bytes);
    for (;;) {
      total += inf_step(st, tab, q, INF_QUEUE);
      if (st.status != INF_OK || st.phase == INF_P_DONE) break;
    }
    bad = bad || st.status != INF_OK;
  }
  return bad ? -1 : total;
}

int host_analysis(int np, const AnalysisArgs& a, int grid) {
  return np_dispatch(np, [&](auto n) { h_analysis<decltype(n)::value>(a, grid); }) ? 0 : -1;
}
int host_gain(int np, const GainArgs& a, int grid) {
  return np_dispatch(np, [&](auto n) {
    grid_stride_visit(a, grid, [&](int64_t p, float& dn1) { return pixel_gain<decltype(n)::value>(a, p, dn1); });
  }) ? 0 : -1;
}
int host_jacobi(int np, const JacobiArgs& a, int grid) {
  return np_dispatch(np, [&](auto n) {
    grid_stride(a.pn > 0 ? a.pn : a.N, grid, a.partials,
                [&](int64_t i) { return pixel_jacobi<decltype(n)::value>(a, a.p0 + i); });
  }) ? 0 : -1;
}
int host_propagate(int np, const PropArgs& a) { return host_pixels<OpPropagate>(np, a); }
int host_invert(int np, const InvertArgs& a) { return host_pixels<OpInvert>(np, a); }
int host_operator(int np, const OperatorArgs& a) { return host_pixels<OpOperator>(np, a); }
int host_gp_operator(int np, const GpOperatorArgs& a) { return host_pixels<OpGpOperatorHost>(np, a); }
int host_hessian(int np, const HessianArgs& a) { return host_pixels<OpHessian>(np, a); }
int host_unpack(int np, const RasterArgs& a) { return host_pixels<OpUnpack>(np, a); }
int host_marginal(int np, const RasterArgs& a) {
  if (a.kind != MARG_PRECISION && a.kind != MARG_COVARIANCE) return -1;
  return host_pixels<OpMarginal>(np, a);
}
int host_product(int np, const ProductArgs& a) { return product_args_ok(np, a) ? host_pixels<OpProduct>(np, a) : -1; }
int host_smooth(int np, const SmoothArgs& a) { return smooth_args_ok(np, a) ? host_pixels<OpSmooth>(np, a) : -1; }
int host_innovation(int np, const InnovationArgs& a) {
  if (!innovation_args_ok(np, a)) return -1;
  return innovation_joint(a) ? host_pixels<OpInnovation<true>>(np, a) : host_pixels<OpInnovation<false>>(np, a);
}
int host_obs_order(const BandDesc* bands, const int32_t* grp, int nb, int G, int64_t N, int32_t* order, bool local) {
  if (G < 1 || G > 3) return -1;
  std::vector<uint8_t> cls((size_t)N);
#pragma omp parallel for schedule(static)
  for (int64_t p = 0; p < N; ++p) cls[p] = (uint8_t)obs_class(bands, grp, nb, G, p);
  // local: each KF_ORD_CHUNK-pixel chunk partitioned in place
  const int64_t span = local ? (int64_t)KF_ORD_CHUNK : N;
  for (int64_t c0 = 0; c0 < N; c0 += span) {
    const int64_t c1 = std::min(N, c0 + span);
    int64_t k = c0;
    for (int c = 0; c < (1 << G); ++c)
      for (int64_t p = c0; p < c1; ++p)
        if (cls[p] == c) order[k++] = (int32_t)p;
  }
  return 0;
}
// Per-chunk Gauss-Newton convergence: each pixel's |dx|^2 in integer quanta
// of its chunk (chunk_quant) summed exactly, as on the device (any order
// gives the same total).
int host_chunk_partials(const ChunkPartialArgs& a) {
#pragma omp parallel for schedule(dynamic, 1)
  for (int c = 0; c < a.n_local; ++c) {
    const int g = a.lc_gid[c];
    if (!a.active[g]) continue;
    const double qi = a.qinv[g];
    int64_t tot = 0;
    for (int sg = a.lc_ptr[c]; sg < a.lc_ptr[c + 1]; ++sg) {
      const int st = a.seg_start[sg], len = a.seg_len[sg];
      for (int i = 0; i < len; ++i) tot += chunk_quant(a.dn[st + i], qi, a.clamp);
    }
    a.part[g] = tot;
  }
  return 0;
}

int host_chunk_decide(const ChunkDecideArgs& a) {
  double mx = 0.0;
  int n_act = 0, px = 0, n_new = 0;
  for (int g = 0; g < a.nc; ++g) {
    const bool was = a.active[g] != 0;
    bool stop = false;
    if (was) {
      int64_t tot = 0;
      for (int r = 0; r < a.world; ++r) tot += a.part_all[(int64_t)r * a.nc + g];
      const double norm = sqrt((double)tot * a.unit);
      mx = std::max(mx, norm);
      stop = chunk_stops(norm, a.n_iter, a.min_iter, a.max_iter, a.tol);
    }
    a.newly[g] = stop ? 1 : 0;
    if (stop) {
      a.active[g] = 0;
      a.iters[g] = a.n_iter;
      ++n_new;
    } else if (was) {
      ++n_act;
      px += a.local_count[g];
    }
  }
  a.info[0] = (double)n_act;
  a.info[1] = mx;
  a.info[2] = (double)px;
  a.info[3] = (double)n_new;
  if (a.px_out) *a.px_out = px;
  return 0;
}

int64_t host_chunk_compact(const ChunkCompactArgs& a) {
  int64_t k = 0;
  const int64_t n_in = visit_bounded(a.n_in, a.n_in, a.n_in_dev);
  for (int64_t q = 0; q < n_in; ++q) {
    const int p = a.order_in ? a.order_in[q] : (int)q;
    const int g = a.chunk_of[p];
    if (a.active[g]) {
      a.order_out[k++] = p;
    } else if (a.newly[g] && a.x_dst) {
      for (int j = 0; j < a.np; ++j) a.x_dst[(int64_t)j * a.ld + p] = a.x_src[(int64_t)j * a.ld + p];
    }
  }
  return k;
}

int host_lut_nearest(const float* lut, int M, int D, const float* x, int64_t N, int64_t ld, int32_t* out) {
#pragma omp parallel for schedule(static)
  for (int64_t p = 0; p < N; ++p) {
    float best = 3.4e38f;
    int bi = 0;
    for (int m = 0; m < M; ++m) {
      float s = 0.f;
      for (int d = 0; d < D; ++d) {
        const float t = lut[m * D + d] - x[d * ld + p];
        s = fmaf(t, t, s);
      }
      if (s < best) { best = s; bi = m; }
    }
    out[p] = bi;
  }
  return 0;
}

// RegTileArgs on the host: the same sweeps over the whole domain (strip plus
// deep halo rows), one at a time (scratch planes), then the strip rows of the
// launch's tile rows are written -- a host run equals the device's tiled pass.
int host_reg_tiled(const RegTileArgs& a) {
  const int64_t w = a.w;
  if (a.nsweep < 1 || a.nsweep > REG_TILE_MAX_SWEEPS || a.w <= 0 || a.h <= 0) return 1;
  if (a.hu < 0 || a.hd < 0 || (a.hu && a.hu < a.nsweep) || (a.hd && a.hd < a.nsweep)) return 1;
  if ((a.hu && !a.halo_up) || (a.hd && !a.halo_dn) || (a.sched && !a.omega_tab)) return 1;
  const int K = reg_tile_nsweep(a);
  bool cheb0 = false;
  if (K > 0) reg_tile_omega(a, 0, cheb0);
  const int H = a.hu + a.h + a.hd;          // domain rows, row 0 = strip row -hu
  const int64_t n = (int64_t)H * w;
  std::vector<float> cur(n), prev(n, 0.f), nxt(n), u(n), v(n);
  const float* ug = a.u + a.j0 * a.ld;
  const float* vg = a.v + a.j0 * a.ld;
  for (int R = 0; R < H; ++R) {
    const int gr = R - a.hu;
    const float *su = ug, *sv = vg, *sz = a.z, *szp = a.zp;
    int64_t off = (int64_t)gr * w;
    if (gr < 0) {
      off = (int64_t)(gr + a.hu) * w;
      su = a.halo_up, sv = a.halo_up + a.halo_plane, sz = a.halo_up + 2 * a.halo_plane;
      szp = a.halo_up + 3 * a.halo_plane;
    } else if (gr >= a.h) {
      off = (int64_t)(gr - a.h) * w;
      su = a.halo_dn, sv = a.halo_dn + a.halo_plane, sz = a.halo_dn + 2 * a.halo_plane;
      szp = a.halo_dn + 3 * a.halo_plane;
    }
    for (int64_t c = 0; c < w; ++c) {
      const int64_t q = (int64_t)R * w + c;
      cur[q] = sz[off + c];
      u[q] = su[off + c];
      v[q] = sv[off + c];
      if ((cheb0 || K == 0) && szp) prev[q] = szp[off + c];
    }
  }
  for (int s = 0; s < K; ++s) {
#pragma omp parallel for schedule(static)
    for (int64_t q = 0; q < n; ++q) {
      const int64_t r = q / w, c = q - r * w;
      const float sn = reg_tile_nsum(cur.data(), q, w, r > 0, r + 1 < H, c > 0, c + 1 < w);
      nxt[q] = reg_tile_step(a, s, sn, u[q], v[q], prev[q]);
    }
    std::swap(prev, cur);
    std::swap(cur, nxt);
  }
  const int tiles_y = (a.h + 63) / 64;
  const int ty0 = a.ty1 == 0 ? 0 : a.ty0, ty1 = a.ty1 == 0 ? tiles_y : a.ty1;
  if (ty0 < 0 || ty1 > tiles_y || ty0 > ty1) return 1;
  const int64_t r_lo = (int64_t)ty0 * 64, r_hi = std::min<int64_t>((int64_t)ty1 * 64, a.h);
  for (int64_t r = r_lo; r < r_hi; ++r) {
    const int64_t src = (r + a.hu) * w;
    std::copy(cur.begin() + src, cur.begin() + src + w, a.z_out + r * w);
    std::copy(prev.begin() + src, prev.begin() + src + w, a.zp_out + r * w);
  }
  return 0;
}

int host_reg_rho(const float* vrow, const StripGeo& g, int64_t N, const RegScheduleArgs& a) {
  if (N <= 0 || g.w <= 0) return 1;
  float m = 0.f;
  for (int64_t p = 0; p < N; ++p) m = std::max(m, reg_rho_term(vrow, g, p));
  a.rho[0] = (double)(m * a.gamma);
  return 0;
}

int host_reg_schedule(const RegScheduleArgs& a) {
  if (a.max_sweeps < 1 || !a.sched || !a.omega_tab || !a.info || !a.rho) return 1;
  double used;
  const int S = reg_cheb_schedule(a.rho[0], a.tol, a.max_sweeps, a.omega_tab, &used);
  a.sched[0] = S - 1;
  a.info[0] = used;
  a.info[1] = (double)S;
  return 0;
}

}  // namespace kf
