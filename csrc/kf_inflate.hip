// kf_inflate.hip — device GeoTIFF tile decoder (kf_inflate.h): inflate one zlib
// stream per 256 x 256 tile, undo the TIFF predictor and place the tile's part
// of the requested window into the dense destination plane.  The ingest side
// then ships compressed tiles over PCIe and the host only reads files.
//
// Launch: one wave per tile, grid = tiles (a 10980^2 band: 1,849).  A workgroup
// is ONE wave, not four: the waves never cooperate, and each needs a 32 KiB
// LDS window (below) beside its tables, so LDS admits four tiles per CU either
// way; one wave per workgroup keeps the allocation static (36 KiB < the 64 KiB
// a kernel can declare) and lets every tile retire on its own.
//
//   decode: lane 0 runs inf_step (Huffman decoding is serial per stream; the
//           tables and the token queue are in LDS) until 64 tokens are queued,
//           a stored block is due or the stream ends; then the whole wave
//           drains the queue in order: one token per lane, a wave scan of the
//           token sizes gives every token its output offset, each run of
//           literals is written by its lanes at once, and each match is copied
//           lane-parallel with src = pos - dist + (j mod dist), which is right
//           for overlapping matches because every source byte precedes pos.
//           Output bytes go
//           to the tile's raw buffer in global memory (fire and forget) AND to
//           a 32 KiB ring in LDS -- DEFLATE's whole window -- which is where
//           matches read: a match costs an LDS round trip, not a global one,
//           and the kernel never reads global memory it has written during
//           the decode.  Within a wave LDS operations execute in program
//           order, so the drain's phases need compiler ordering only
//           (wavefront-scope fences), no waits.  Adler-32 partial sums are
//           kept per lane in 64 bits and combined as dfl_adler does.
//   place:  after the stores have landed (s_waitcnt vmcnt(0)), the wave reads
//           the raw tile back row by row: 16 bytes per lane, the predictor by a
//           wave scan (predictor 2: 16-bit prefix sum; predictor 3: byte
//           prefix sum, then the byte planes are regrouped through LDS), and
//           16-byte stores of the columns inside the window where the
//           destination is aligned, element stores at the window's edges.
//           A failed tile's part of the window is zeroed.
#include <hip/hip_runtime.h>

#include "kf_inflate.h"
#include "kf_launch.h"

namespace kf {

namespace {

struct InfCtl {
  int32_t ntok, status, phase;
  uint32_t sto_off, sto_len, adler;
};

// compiler ordering between the phases of a drain (a wave's LDS operations
// execute in order: no wait is needed)
__device__ __forceinline__ void wave_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct alignas(16) Vec16 {
  uint32_t w[4];
};

}  // namespace

__global__ __launch_bounds__(64) void inf_tile_kernel(InfArgs a) {
  const int tile = blockIdx.x, lane = threadIdx.x;
  __shared__ __attribute__((aligned(16))) uint8_t ring[INF_WINDOW];
  __shared__ InfTables tab;
  __shared__ uint32_t q[INF_QUEUE];
  __shared__ InfCtl ctl;
  constexpr uint32_t MASK = INF_WINDOW - 1;
  const int T = a.tile, e = a.elem_bytes;
  const int64_t tile_bytes = (int64_t)T * T * e;
  const int64_t stride = inf_scratch_stride(a.raw_bytes, T, e);
  uint8_t* raw = a.scratch + (int64_t)tile * stride;
  const uint32_t n = (uint32_t)a.raw_bytes;
  const int64_t off = a.offs[tile], sz = a.sizes[tile];
  const bool in_range = off >= 0 && sz >= 0 && sz <= 0x7FFFFFFF && off <= a.comp_bytes && sz <= a.comp_bytes - off;
  int32_t status = in_range ? INF_OK : INF_TRUNCATED;

  if (in_range) {
    InfState st;                         // lane 0's copy is the live one
    inf_init(st, a.comp + off, (uint32_t)sz, n);
    uint32_t pos = 0;                    // bytes written so far (the same in every lane)
    uint64_t s1 = 0, s2 = 0;
    for (;;) {                           // every round takes >= 1 bit of the stream or ends it
      if (lane == 0) {
        ctl.ntok = inf_step(st, tab, q, INF_QUEUE);
        ctl.status = st.status;
        ctl.phase = st.phase;
        ctl.sto_off = st.sto_off;
        ctl.sto_len = st.sto_len;
        ctl.adler = st.adler;
      }
      wave_order();
      const int ntok = ctl.ntok;
      KF_DCHECK(ntok >= 0 && ntok <= INF_QUEUE);
      const uint32_t tk = lane < ntok ? q[lane] : 0u;
      const bool is_match = lane < ntok && inf_tok_is_match(tk);
      const uint32_t size = lane < ntok ? (is_match ? inf_tok_len(tk) : 1u) : 0u;
      uint32_t x = size;                 // inclusive scan of the token sizes
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
      }
      const uint32_t start = pos + x - size;
      KF_DCHECK((uint64_t)start + size <= n);
      // The literals between two matches are written just before the later
      // match, not all at once: a literal's ring slot is that of the byte
      // 32 KiB before it, which an EARLIER match of this round may still read.
      auto literals = [&](int after, int before) {
        if (lane > after && lane < before && lane < ntok && !is_match) {
          ring[start & MASK] = (uint8_t)tk;
          raw[start] = (uint8_t)tk;
          inf_adler_add(s1, s2, tk & 0xFFu, start, n);
        }
        wave_order();
      };
      uint64_t m = __ballot(is_match);
      int prev = -1;
      while (m) {                        // matches in stream order (m is the same in every lane)
        const int l = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        literals(prev, l);
        prev = l;
        const uint32_t mt = __shfl(tk, l, 64), P = __shfl(start, l, 64);
        const uint32_t L = inf_tok_len(mt), D = inf_tok_dist(mt);
        KF_DCHECK(D <= P && (uint64_t)P + L <= n);
        for (uint32_t j = lane; j < L; j += 64) {
          const uint32_t k = D >= L ? j : j % D;
          const uint32_t b = ring[(P - D + k) & MASK];
          ring[(P + j) & MASK] = (uint8_t)b;
          raw[P + j] = (uint8_t)b;
          inf_adler_add(s1, s2, b, P + j, n);
        }
        wave_order();
      }
      literals(prev, INF_QUEUE);
      pos += __shfl(x, 63, 64);
      const uint32_t slen = ctl.sto_len, soff = ctl.sto_off;
      KF_DCHECK((uint64_t)pos + slen <= n && (uint64_t)soff + slen <= (uint64_t)sz);
      for (uint32_t j = lane; j < slen; j += 64) {   // a stored block's payload
        const uint32_t b = st.in[soff + j];
        ring[(pos + j) & MASK] = (uint8_t)b;
        raw[pos + j] = (uint8_t)b;
        inf_adler_add(s1, s2, b, pos + j, n);
      }
      pos += slen;
      const int32_t s = ctl.status, ph = ctl.phase;
      wave_order();                      // ctl and q are read before lane 0 writes them again
      if (s != INF_OK || ph == INF_P_DONE) {
        status = s;
        break;
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      s1 += __shfl_down(s1, o, 64);
      s2 += __shfl_down(s2, o, 64);
    }
    const uint32_t adler = dfl_adler(__shfl(s1, 0, 64), __shfl(s2, 0, 64), (int64_t)n);
    if (status == INF_OK && adler != ctl.adler) status = INF_BAD_ADLER;
    for (int64_t i = a.raw_bytes + lane; i < tile_bytes; i += 64) raw[i] = 0;   // a raw size short of a tile
  }
  if (lane == 0) a.status[tile] = status;

  // ---- place: the tile's part of the window
  const int64_t gy0 = (int64_t)a.tile_rc[2 * tile] * T, gx0 = (int64_t)a.tile_rc[2 * tile + 1] * T;
  const int64_t ya = gy0 > a.r0 ? gy0 : a.r0, yb = gy0 + T < a.r1 ? gy0 + T : a.r1;
  const int64_t xa = gx0 > a.c0 ? gx0 : a.c0, xb = gx0 + T < a.c1 ? gx0 + T : a.c1;
  if (ya >= yb || xa >= xb) return;
  uint8_t* dst = static_cast<uint8_t*>(a.dst);
  if (status != INF_OK) {
    const int64_t w = xb - xa, cells = (yb - ya) * w;
    for (int64_t i = lane; i < cells; i += 64) {
      const int64_t y = ya + i / w, xx = xa + i % w;
      const int64_t at = (y - a.r0) * a.ld + (xx - a.c0);
      KF_DCHECK(at >= 0 && at < (a.r1 - a.r0) * a.ld);
      if (e == 2) reinterpret_cast<uint16_t*>(dst)[at] = 0;
      else reinterpret_cast<uint32_t*>(dst)[at] = 0u;
    }
    return;
  }
  // the decode's stores have to land before other lanes read them back
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

  if (e == 2) {
    // two rows per round: 32 lanes x 8 samples (16 bytes) each
    const int half = lane >> 5, l32 = lane & 31;
    for (int64_t yy = ya; yy < yb; yy += 2) {
      const int64_t y = yy + half;
      const bool live = y < yb;
      Vec16 v = {{0u, 0u, 0u, 0u}};
      if (live) {
        KF_DCHECK((y - gy0) * 512 + l32 * 16 + 16 <= stride);
        v = *reinterpret_cast<const Vec16*>(raw + (y - gy0) * 512 + l32 * 16);
      }
      uint32_t sm[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) sm[k] = (v.w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
      if (a.predictor == 2) {
#pragma unroll
        for (int k = 1; k < 8; ++k) sm[k] += sm[k - 1];
        uint32_t x = sm[7];              // scan of the lanes' sums within the row (mod 2^16 at the end)
        for (int o = 1; o < 32; o <<= 1) {
          const uint32_t u = __shfl_up(x, o, 32);
          if (l32 >= o) x += u;
        }
        const uint32_t before = x - sm[7];
#pragma unroll
        for (int k = 0; k < 8; ++k) sm[k] = (sm[k] + before) & 0xFFFFu;
      }
      if (!live) continue;
      const int64_t gx = gx0 + l32 * 8;
      uint16_t* d = reinterpret_cast<uint16_t*>(dst) + (y - a.r0) * a.ld + (gx - a.c0);
      if (gx >= xa && gx + 8 <= xb && (reinterpret_cast<uintptr_t>(d) & 15u) == 0) {
        Vec16 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o.w[k] = sm[2 * k] | (sm[2 * k + 1] << 16);
        *reinterpret_cast<Vec16*>(d) = o;
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (gx + k >= xa && gx + k < xb) d[k] = (uint16_t)sm[k];
      }
    }
    return;
  }
  // float32: one row per round, 64 lanes x 4 samples (16 bytes)
  for (int64_t y = ya; y < yb; ++y) {
    KF_DCHECK((y - gy0) * 1024 + lane * 16 + 16 <= stride);
    Vec16 v = *reinterpret_cast<const Vec16*>(raw + (y - gy0) * 1024 + lane * 16);
    if (a.predictor == 3) {
      // bytes lane * 16 .. + 15 of the predicted row: prefix sum mod 256 ...
      uint32_t b[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) b[k] = (v.w[k >> 2] >> (8 * (k & 3))) & 0xFFu;
#pragma unroll
      for (int k = 1; k < 16; ++k) b[k] += b[k - 1];
      uint32_t x = b[15];
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(x, o, 64);
        if (lane >= o) x += u;
      }
      const uint32_t before = x - b[15];
      Vec16 p;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        p.w[k] = ((b[4 * k] + before) & 0xFFu) | (((b[4 * k + 1] + before) & 0xFFu) << 8) |
                 (((b[4 * k + 2] + before) & 0xFFu) << 16) | (((b[4 * k + 3] + before) & 0xFFu) << 24);
      // ... then sample c = plane 0 byte c (most significant) .. plane 3 byte c, through LDS
      *reinterpret_cast<Vec16*>(ring + lane * 16) = p;
      wave_order();
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = lane * 4 + k;
        v.w[k] = ((uint32_t)ring[c] << 24) | ((uint32_t)ring[256 + c] << 16) | ((uint32_t)ring[512 + c] << 8) |
                 (uint32_t)ring[768 + c];
      }
      wave_order();
    }
    const int64_t gx = gx0 + lane * 4;
    uint32_t* d = reinterpret_cast<uint32_t*>(dst) + (y - a.r0) * a.ld + (gx - a.c0);
    if (gx >= xa && gx + 4 <= xb && (reinterpret_cast<uintptr_t>(d) & 15u) == 0) {
      *reinterpret_cast<Vec16*>(d) = v;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (gx + k >= xa && gx + k < xb) d[k] = v.w[k];
    }
  }
}

hipError_t dev_inflate_tiles(const InfArgs& a, hipStream_t s) {
  if (!inf_args_ok(a) || !a.scratch || (reinterpret_cast<uintptr_t>(a.scratch) & 15u)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(inf_tile_kernel, dim3(a.ntiles), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace kf
