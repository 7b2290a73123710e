// kf_deflate.hip — device GeoTIFF tile encoder (kf_deflate.h): predictor 3 +
// one zlib stream per 256 x 256 float32 tile (fixed Huffman: dfl_tile_kernel,
// described first; a dynamic table per tile: dfl_tile_dyn_kernel, which also
// holds both modes of the scaled 16-bit format), then the tiles
// packed back to back. Reference-cadence output (observations.py:354-394)
// then ships compressed tiles to the host instead of raw planes, and the host
// writer only writes files.
//
// Launch: one workgroup of 256 threads per tile (thread = tile row), grid =
// planes x tiles (a 10980^2 x 7 date: 12,943 workgroups, 50 per CU).
//   pass 1: each thread encodes its row once, into a word-aligned scratch
//           slot of its own, with the Adler-32 partials; a workgroup scan
//           gives every row its bit offset in the stream;
//   pass 2: each thread moves its row's words to that offset (a shift).
//           Words wholly inside a row's range are stored directly; the one
//           word a row shares with the next (its tail) goes through LDS and is
//           OR-ed into the next row's head word, so no atomics and no zeroed
//           buffer are needed (every row emits >= 65 bits, so a word never
//           spans three rows).
// Thread 0 prepends the zlib header and the block header, thread 255 appends
// the end-of-block code, the byte padding and the Adler-32 (big-endian).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "kf_deflate.h"
#include "kf_launch.h"

namespace kf {

__global__ __launch_bounds__(DFL_TILE) void dfl_tile_kernel(DflArgs a) {
  const int tile = blockIdx.x;
  const int per = a.tiles_x * a.tiles_y;
  const int plane = tile / per, tt = tile - plane * per;
  const int ty = tt / a.tiles_x, tx = tt - ty * a.tiles_x;
  const int r = threadIdx.x;
  const int64_t y = (int64_t)ty * DFL_TILE + r;
  const int x0 = tx * DFL_TILE;
  const bool rin = y < a.H;
  const int ncol = a.W - x0 < DFL_TILE ? a.W - x0 : DFL_TILE;
  const float* rowp = a.src + (int64_t)plane * a.plane_ld + (rin ? y : 0) * a.W + x0;
  // the row's samples in groups of 16: one burst of independent loads into this
  // thread's LDS line per group (the encoder reads columns in order, 4 passes
  // over the row, one per byte plane), instead of one dependent load per byte
  __shared__ uint32_t line[DFL_TILE][17];
  auto row = [&](int c) -> uint32_t {
    if ((c & 15) == 0) {
      uint32_t v[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = (rin && c + j < ncol) ? __float_as_uint(rowp[c + j]) : 0u;
#pragma unroll
      for (int j = 0; j < 16; ++j) line[r][j] = v[j];
    }
    return line[r][c & 15];
  };
  const int64_t rest = DFL_RAW - (int64_t)r * DFL_ROW;

  // pass 1: the row's bit string into its own word-aligned scratch slot (one
  // encode of the row), its length and Adler partials
  uint32_t* rs = reinterpret_cast<uint32_t*>(a.scratch) + ((int64_t)tile * DFL_TILE + r) * DFL_ROW_WORDS;
  uint64_t nbits = 0, s1 = 0, s2 = 0;
  {
    uint64_t acc = 0;
    int nacc = 0, wi = 0;
    dfl_encode_row(row, rest, [&](uint32_t bits, int len) {
      acc |= (uint64_t)bits << nacc;
      nacc += len;
      nbits += (uint64_t)len;
      if (nacc >= 32) {
        rs[wi++] = (uint32_t)acc;
        acc >>= 32;
        nacc -= 32;
      }
    }, s1, s2);
    if (nacc > 0) rs[wi] = (uint32_t)acc;
  }
  KF_DCHECK(nbits >= 64 && nbits <= 32u * DFL_ROW_WORDS);

  __shared__ uint64_t scan[DFL_TILE];
  __shared__ uint64_t red1[DFL_TILE / 64], red2[DFL_TILE / 64];
  __shared__ uint32_t tail[DFL_TILE];
  scan[r] = nbits;
  uint64_t w1 = s1, w2 = s2;
  for (int o = 32; o > 0; o >>= 1) {
    w1 += __shfl_down(w1, o, 64);
    w2 += __shfl_down(w2, o, 64);
  }
  if ((r & 63) == 0) {
    red1[r >> 6] = w1;
    red2[r >> 6] = w2;
  }
  __syncthreads();
  // inclusive Hillis-Steele scan of the row bit counts
  for (int o = 1; o < DFL_TILE; o <<= 1) {
    const uint64_t v = r >= o ? scan[r - o] : 0;
    __syncthreads();
    scan[r] += v;
    __syncthreads();
  }
  const uint64_t start = DFL_HEAD_BITS + scan[r] - nbits;
  uint64_t t1 = 0, t2 = 0;
#pragma unroll
  for (int w = 0; w < DFL_TILE / 64; ++w) {
    t1 += red1[w];
    t2 += red2[w];
  }
  const uint32_t adler = dfl_adler(t1, t2, DFL_RAW);

  // pass 2: the row's words shifted to its bit offset in the stream.  Words
  // wholly inside the row's range are stored; the word shared with the next
  // row goes through LDS (every row emits >= 65 bits: no word spans 3 rows)
  uint32_t* out = reinterpret_cast<uint32_t*>(a.out + (int64_t)tile * DFL_BOUND);
  const bool shared_left = r > 0 && (start & 31u) != 0;
  uint64_t wi = start >> 5;
  uint64_t acc = 0;
  int nacc = (int)(start & 31u);
  if (r == 0) {
    acc = 0x0178u | (1u << 16) | (1u << 17);   // 78 01, BFINAL = 1, BTYPE = 01 (fixed Huffman)
    nacc = DFL_HEAD_BITS;
  }
  uint32_t head = 0;
  bool first = true;
  auto put = [&](uint32_t v) {
    if (first && shared_left) head = v;
    else out[wi] = v;
    first = false;
    ++wi;
  };
  auto sink = [&](uint32_t bits, int len) {
    acc |= (uint64_t)bits << nacc;
    nacc += len;
    while (nacc >= 32) {
      put((uint32_t)acc);
      acc >>= 32;
      nacc -= 32;
    }
  };
  const int full = (int)(nbits >> 5), part = (int)(nbits & 31u);
  for (int k = 0; k < full; ++k) sink(rs[k], 32);
  if (part) sink(rs[full] & ((1u << part) - 1u), part);
  if (r == DFL_TILE - 1) {
    sink(0u, 7);                                       // end of block (code 256: 7 zero bits)
    const int pad = (8 - (int)(((wi << 5) + nacc) & 7u)) & 7;
    if (pad) sink(0u, pad);
    for (int k = 3; k >= 0; --k) sink((adler >> (8 * k)) & 0xFFu, 8);   // Adler-32, big-endian bytes
    const uint64_t end_bits = (wi << 5) + nacc;
    if (nacc > 0) out[wi] = (uint32_t)acc;             // the stream's last word: nobody shares it
    a.sizes[tile] = (uint32_t)(end_bits >> 3);
  } else if (nacc > 0) {
    tail[r] = (uint32_t)acc;                           // shared with row r + 1's head word
  }
  __syncthreads();
  if (shared_left) out[start >> 5] = head | tail[r - 1];
}

// Dynamic-Huffman mode (kf_deflate.h): the same launch shape, three passes.
//   count:  each thread tokenises its row into a per-wave LDS histogram
//           (integer LDS adds: any order gives the same counts) and sums its
//           Adler partials;
//   build:  the used symbols are ranked by (frequency, index), one or two
//           symbols per thread; lane 0 derives the code lengths, the codes and
//           the header, compares the block with the fixed one and leaves the
//           chosen table in LDS;
//   encode: each thread tokenises its row again, with the table, into its
//           scratch slot (DFL_ROW_WORDS_DYN words: up to 15 bits per byte);
//           a workgroup scan gives the bit offsets, then the shift.
// A row here can be shorter than a word (a constant tile: ~33 bits), so any
// number of rows may share a word: every word that a row covers only in part
// is zeroed first and then receives the rows' disjoint bit ranges by atomic OR
// (order-independent); words wholly inside a row are stored directly.
//
// FMT = DFL_FMT_U16 (scaled 16-bit samples, predictor 2): the row load
// quantises each burst of 16 samples (dfl_quantise), differences them as
// 16-bit words against the previous column carried in a register, and leaves
// the 16 differences in the thread's uint16 LDS line; the tokeniser then reads
// the row's 512 bytes in order, one pass over the columns.  Saturated samples
// are summed per thread in the first pass over the row, then per wave, and one
// atomicAdd per wave goes to the plane's counter.  A constant 16-bit row is
// ~39 bits with the fixed codes too, so the fixed mode of this format
// (DYN = false: no count and build passes, the fixed codes computed directly)
// runs through this kernel's merge as well, not dfl_tile_kernel's.
template <int FMT, bool DYN>
__global__ __launch_bounds__(DFL_TILE) void dfl_tile_dyn_kernel(DflArgs a) {
  static_assert(DYN || FMT == DFL_FMT_U16, "float32 fixed mode: dfl_tile_kernel");
  constexpr int ROW = dfl_row_len(FMT);
  constexpr int64_t RAW = dfl_raw(FMT), BOUND = dfl_bound(FMT);
  constexpr int ROW_WORDS = dfl_row_words(FMT, DYN);
  const int tile = blockIdx.x;
  const int per = a.tiles_x * a.tiles_y;
  const int plane = tile / per, tt = tile - plane * per;
  const int ty = tt / a.tiles_x, tx = tt - ty * a.tiles_x;
  const int r = threadIdx.x;
  const int64_t y = (int64_t)ty * DFL_TILE + r;
  const int x0 = tx * DFL_TILE;
  const bool rin = y < a.H;
  const int ncol = a.W - x0 < DFL_TILE ? a.W - x0 : DFL_TILE;
  const float* rowp = a.src + (int64_t)plane * a.plane_ld + (rin ? y : 0) * a.W + x0;
  // float32: the samples' bits; 16-bit: the burst's differences (18 uint16 =
  // 9 words per line: an odd word stride)
  using line_t = typename std::conditional<FMT == DFL_FMT_U16, uint16_t, uint32_t>::type;
  __shared__ line_t line[DFL_TILE][FMT == DFL_FMT_U16 ? 18 : 17];
  float qa = 0.f, qb = 0.f;
  if constexpr (FMT == DFL_FMT_U16) {
    qa = a.qa[plane];
    qb = a.qb[plane];
  }
  uint32_t sat = 0, qprev = 0;
  auto row = [&](int i) -> uint32_t {
    if constexpr (FMT == DFL_FMT_U16) {
      // i: byte of the row's differences, ascending; a burst every 32 bytes
      if ((i & 31) == 0) {
        const int c = i >> 1;
        float v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = (rin && c + j < ncol) ? rowp[c + j] : 0.f;
        uint32_t p = c ? qprev : 0u;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const uint32_t q = (rin && c + j < ncol) ? dfl_quantise(v[j], qa, qb, sat) : 0u;
          line[r][j] = (uint16_t)(q - p);
          p = q;
        }
        qprev = p;
      }
      return ((uint32_t)line[r][(i >> 1) & 15] >> (8 * (i & 1))) & 0xFFu;
    } else {
      const int c = i;
      if ((c & 15) == 0) {
        uint32_t v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = (rin && c + j < ncol) ? __float_as_uint(rowp[c + j]) : 0u;
#pragma unroll
        for (int j = 0; j < 16; ++j) line[r][j] = v[j];
      }
      return line[r][c & 15];
    }
  };
  const int64_t rest = RAW - (int64_t)r * ROW;

  __shared__ uint32_t hist[DYN ? DFL_TILE / 64 : 1][DYN ? DFL_NSYM : 1];
  __shared__ DflTable tab;
  __shared__ DflWork work;
  __shared__ int used;
  __shared__ uint64_t scan[DFL_TILE];
  __shared__ uint64_t red1[DFL_TILE / 64], red2[DFL_TILE / 64];

  uint64_t s1 = 0, s2 = 0;
  if constexpr (DYN) {
    // count
    for (int i = r; i < (DFL_TILE / 64) * DFL_NSYM; i += DFL_TILE) (&hist[0][0])[i] = 0;
    if (r == 0) used = 0;
    __syncthreads();
    {
      uint32_t* h = hist[r >> 6];
      dfl_tokenise_row<FMT>(row, rest, [&](uint32_t v, int L) { atomicAdd(&h[dfl_token_symbol(v, L)], 1u); }, s1, s2);
    }
  }

  // encode (DYN = false): the fixed codes, the Adler partials in the same pass
  uint32_t* rs = reinterpret_cast<uint32_t*>(a.scratch) + ((int64_t)tile * DFL_TILE + r) * ROW_WORDS;
  uint64_t nbits = 0;
  if constexpr (!DYN) {
    uint64_t acc = 0;
    int nacc = 0, wi = 0;
    dfl_encode_row<FMT>(row, rest, [&](uint32_t bits, int len) {
      acc |= (uint64_t)bits << nacc;
      nacc += len;
      nbits += (uint64_t)len;
      if (nacc >= 32) {
        rs[wi++] = (uint32_t)acc;
        acc >>= 32;
        nacc -= 32;
      }
    }, s1, s2);
    if (nacc > 0) rs[wi] = (uint32_t)acc;
  }
  const uint32_t nsat = sat;      // one pass over the row so far: every sample counted once

  uint64_t w1 = s1, w2 = s2;
  uint32_t w3 = nsat;
  for (int o = 32; o > 0; o >>= 1) {
    w1 += __shfl_down(w1, o, 64);
    w2 += __shfl_down(w2, o, 64);
    if constexpr (FMT == DFL_FMT_U16) w3 += __shfl_down(w3, o, 64);
  }
  if ((r & 63) == 0) {
    red1[r >> 6] = w1;
    red2[r >> 6] = w2;
    if constexpr (FMT == DFL_FMT_U16)
      if (w3 != 0 && a.sat != nullptr) atomicAdd(&a.sat[plane], w3);
  }
  __syncthreads();

  if constexpr (DYN) {
    uint32_t* freq = hist[0];
    for (int i = r; i < DFL_NSYM; i += DFL_TILE) {
      uint32_t f = 0;
#pragma unroll
      for (int w = 0; w < DFL_TILE / 64; ++w) f += hist[w][i];
      freq[i] = i == 256 ? 1u : f;               // the end-of-block code
    }
    __syncthreads();

    // build
    for (int i = r; i < DFL_NSYM; i += DFL_TILE) {
      const int rk = dfl_rank(freq, DFL_NSYM, i);
      if (rk >= 0) {
        work.sorted[rk] = (uint16_t)i;
        atomicAdd(&used, 1);
      }
    }
    __syncthreads();
    if (r == 0) dfl_choose_table(freq, used, false, tab, work);
    __syncthreads();

    // encode: the row's bit string into its own word-aligned scratch slot
    uint64_t acc = 0, u1, u2;
    int nacc = 0, wi = 0;
    dfl_tokenise_row<FMT>(row, rest, [&](uint32_t v, int L) {
      uint32_t bits;
      int len;
      dfl_table_token(tab, v, L, bits, len);
      acc |= (uint64_t)bits << nacc;
      nacc += len;
      nbits += (uint64_t)len;
      if (nacc >= 32) {
        rs[wi++] = (uint32_t)acc;
        acc >>= 32;
        nacc -= 32;
      }
    }, u1, u2);
    if (nacc > 0) rs[wi] = (uint32_t)acc;
  }
  KF_DCHECK(nbits >= 1 && nbits <= 32u * (ROW_WORDS - 1));

  scan[r] = nbits;
  __syncthreads();
  // inclusive Hillis-Steele scan of the row bit counts
  for (int o = 1; o < DFL_TILE; o <<= 1) {
    const uint64_t v = r >= o ? scan[r - o] : 0;
    __syncthreads();
    scan[r] += v;
    __syncthreads();
  }
  uint64_t t1 = 0, t2 = 0;
#pragma unroll
  for (int w = 0; w < DFL_TILE / 64; ++w) {
    t1 += red1[w];
    t2 += red2[w];
  }
  const uint32_t adler = dfl_adler(t1, t2, RAW);

  // this thread's bit range [b0, b1) of the stream: its row, with the zlib and
  // block headers in front of row 0 and the end-of-block code, the byte
  // padding and the Adler-32 behind row 255
  const uint32_t head_bits = DYN ? tab.head_bits : 3u;
  const uint64_t start = 16u + head_bits + scan[r] - nbits;
  const uint64_t b0 = r == 0 ? 0 : start;
  uint64_t b1 = start + nbits;
  const int eobl = DYN ? tab.len[256] : 7;
  if (r == DFL_TILE - 1) b1 = ((b1 + eobl + 7u) & ~(uint64_t)7u) + 32u;
  KF_DCHECK(r != DFL_TILE - 1 || b1 <= 8u * (uint64_t)BOUND);
  uint32_t* out = reinterpret_cast<uint32_t*>(a.out + (int64_t)tile * BOUND);
  if (b0 & 31u) out[b0 >> 5] = 0u;
  if (b1 & 31u) out[(b1 - 1) >> 5] = 0u;
  __threadfence();
  __syncthreads();

  const bool shared_left = (b0 & 31u) != 0;
  uint64_t wi = b0 >> 5;
  uint64_t acc = 0;
  int nacc = (int)(b0 & 31u);
  bool first = true;
  auto sink = [&](uint32_t bits, int len) {
    acc |= (uint64_t)bits << nacc;
    nacc += len;
    while (nacc >= 32) {
      if (first && shared_left) atomicOr(&out[wi], (uint32_t)acc);
      else out[wi] = (uint32_t)acc;
      first = false;
      ++wi;
      acc >>= 32;
      nacc -= 32;
    }
  };
  if (r == 0) {
    sink(0x0178u, 16);                                   // 78 01
    if constexpr (DYN) dfl_write_block_header(tab, sink);
    else sink(3u, 3);                                    // BFINAL = 1, BTYPE = 01 (fixed Huffman)
  }
  const int full = (int)(nbits >> 5), part = (int)(nbits & 31u);
  for (int k = 0; k < full; ++k) sink(rs[k], 32);
  if (part) sink(rs[full] & ((1u << part) - 1u), part);
  if (r == DFL_TILE - 1) {
    sink(DYN ? (uint32_t)tab.code[256] : 0u, eobl);      // end of block
    const int pad = (8 - (int)(((wi << 5) + nacc) & 7u)) & 7;
    if (pad) sink(0u, pad);
    for (int k = 3; k >= 0; --k) sink((adler >> (8 * k)) & 0xFFu, 8);   // Adler-32, big-endian bytes
    a.sizes[tile] = (uint32_t)(b1 >> 3);
  }
  KF_DCHECK((wi << 5) + (uint64_t)nacc == b1);
  if (nacc > 0) atomicOr(&out[wi], (uint32_t)acc);       // the last word: covered in part
}

// tile t's stream (sizes[t] bytes at t * bound) -> packed + offs[t]
__global__ __launch_bounds__(256) void dfl_pack_kernel(const uint8_t* scratch, const uint32_t* sizes,
                                                       const int64_t* offs, uint8_t* packed, int64_t bound) {
  const int t = blockIdx.x;
  const uint32_t n = sizes[t];
  const uint8_t* src = scratch + (int64_t)t * bound;
  uint8_t* dst = packed + offs[t];
  for (uint32_t i = threadIdx.x; i < n; i += 256) dst[i] = src[i];
}

hipError_t dev_deflate_tiles(const DflArgs& a, hipStream_t s) {
  const int n = a.nplanes * a.tiles_x * a.tiles_y;
  if (n <= 0 || a.W <= 0 || a.H <= 0) return hipErrorInvalidValue;
  const dim3 g(n), b(DFL_TILE);
  if (a.fmt == DFL_FMT_F32) {
    if (a.mode == DFL_MODE_FIXED) hipLaunchKernelGGL(dfl_tile_kernel, g, b, 0, s, a);
    else if (a.mode == DFL_MODE_DYNAMIC)
      hipLaunchKernelGGL((dfl_tile_dyn_kernel<DFL_FMT_F32, true>), g, b, 0, s, a);
    else return hipErrorInvalidValue;
  } else if (a.fmt == DFL_FMT_U16 && a.qa != nullptr && a.qb != nullptr) {
    if (a.mode == DFL_MODE_FIXED) hipLaunchKernelGGL((dfl_tile_dyn_kernel<DFL_FMT_U16, false>), g, b, 0, s, a);
    else if (a.mode == DFL_MODE_DYNAMIC)
      hipLaunchKernelGGL((dfl_tile_dyn_kernel<DFL_FMT_U16, true>), g, b, 0, s, a);
    else return hipErrorInvalidValue;
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t dev_deflate_pack(const uint8_t* scratch, const uint32_t* sizes, const int64_t* offs, uint8_t* packed,
                            int ntiles, hipStream_t s, int64_t bound) {
  if (ntiles <= 0 || bound <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dfl_pack_kernel, dim3(ntiles), dim3(256), 0, s, scratch, sizes, offs, packed, bound);
  return hipGetLastError();
}

}  // namespace kf
