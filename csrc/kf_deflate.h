// kf_deflate.h — GeoTIFF tile encoding on the device: the TIFF floating-point
// predictor (predictor 3) and a zlib stream per 256 x 256 float32 tile, for
// reference-cadence output (every parameter's mean and uncertainty raster at
// every timestep, observations.py:354-394 / linear_kf.py:211-212).
//
// One tile = 256 rows of 1024 predicted bytes = one zlib stream (TIFF
// compression 8): the 2-byte header 78 01, ONE final DEFLATE block with the
// fixed Huffman codes (RFC 1951 §3.2.6), the Adler-32 of the predicted bytes.
// The LZ77 part is run-length only (distance 1, lengths 3..258), the same
// match family as zlib's Z_RLE strategy that ``--out-fast`` selects on the
// host, and every row starts with a literal: each row's symbols depend on
// that row alone, so one thread encodes one row.  The row encoder below is
// the source both the gfx950 kernel (kf_deflate.hip: one workgroup per tile,
// bit offsets by a workgroup scan) and the host runner (tests, CPU builds)
// execute, so their streams are bit-identical.
//
// Dynamic-Huffman mode (DFL_MODE_DYNAMIC): the same tokens, but the tile's one
// block is BTYPE = 10 (RFC 1951 §3.2.7) with a literal/length code built from
// the tile's own token histogram, whenever that block is strictly smaller than
// the fixed one (both sizes are exact before a bit is emitted); otherwise the
// fixed block is emitted, bit for bit.  Everything that decides a bit is below
// and is integer arithmetic; wherever a tie can occur the order is total:
//   * symbols are sorted ascending by (frequency, symbol index); only symbols
//     with a non-zero frequency take part (dfl_rank);
//   * the Huffman merge is the two-queue one over that sorted list: each step
//     takes the two lightest nodes, and of a leaf and an internal node of equal
//     weight it takes the leaf; internal nodes are taken in creation order;
//   * depths above the limit (15; 7 for the code-length code) are folded into
//     the limit, then, until the Kraft sum is exactly 1, one code of the
//     longest length is dropped and one code of the longest shorter length L
//     is replaced by two of length L + 1 (counts per length only);
//   * lengths go to symbols by the sorted order: shortest to the last (most
//     frequent, highest index among equals);
//   * codes are canonical (RFC 1951 §3.2.2), stored bit-reversed;
//   * the code lengths (literal/length lengths up to the last used symbol, at
//     least 257, then the one distance code of length 1) are one sequence,
//     run-length coded greedily: zero runs as 18 (11..138, longest first) then
//     17 (3..10) then single zeros; a non-zero run as the length itself, then
//     16 (6 at a time while >= 3 remain), then the length itself.
// A row then costs anything from ~33 bits (a constant tile) to 15 bits per byte
// (a noise row in a quiet tile): DFL_ROW_WORDS_DYN sizes the row scratch, and
// the kernel's merge of the rows' partial words allows any number of rows in a
// word.
//
// Predictor 3 (TIFF Technical Note 3): each row's samples are split into byte
// planes, most significant byte first, and the 4 x 256 bytes are differenced
// (d[0] = r[0], d[i] = r[i] - r[i - 1] mod 256).
//
// Scaled 16-bit samples (DFL_FMT_U16, opt-in): the same streams over rows of
// 512 bytes, the float samples quantised on the way in (dfl_quantise) and
// differenced as 16-bit words (TIFF predictor 2); see DFL_FMT_* below.
#pragma once
#include <stdint.h>
#include "kf_core.h"

namespace kf {

constexpr int DFL_TILE = 256;                                   // tile edge (pixels)
constexpr int DFL_ROW = DFL_TILE * 4;                           // predicted bytes per row
constexpr int64_t DFL_RAW = (int64_t)DFL_TILE * DFL_ROW;        // 262144 bytes per tile
// worst case: header 2 + (19 + 9 bits per byte + 7 EOB + 7 pad) / 8 + Adler 4, rounded to 16
constexpr int64_t DFL_BOUND = ((2 + (19 + 9 * DFL_RAW + 14) / 8 + 4) + 15) / 16 * 16;
constexpr int DFL_HEAD_BITS = 19;   // zlib header (16) + BFINAL/BTYPE (3)
// scratch words of one encoded row (9 bits per byte at most, plus a partial word)
constexpr int DFL_ROW_WORDS = (9 * DFL_ROW + 31) / 32 + 1;
constexpr uint32_t DFL_ADLER_MOD = 65521u;
// DflArgs.mode.  DFL_MODE_DYNAMIC_FORCE_FIXED runs the dynamic path with the
// per-tile choice forced to the fixed block (host runner only: the tests pin
// the fallback to the fixed-mode bytes with it)
constexpr int DFL_MODE_FIXED = 0, DFL_MODE_DYNAMIC = 1, DFL_MODE_DYNAMIC_FORCE_FIXED = 2;
constexpr int DFL_NSYM = 286;       // literal/length symbols
constexpr int DFL_NCL = 19;         // code-length symbols
constexpr int DFL_MAX_BITS = 15, DFL_MAX_CL_BITS = 7;
// dynamic mode: a literal costs 15 bits at most, and a match (>= 3 bytes) at
// most 15 + 5 extra + 5 distance bits (fixed fallback) = 25 <= 45
constexpr int DFL_ROW_WORDS_DYN = (DFL_MAX_BITS * DFL_ROW + 31) / 32 + 1;
static_assert(32 * (DFL_ROW_WORDS_DYN - 1) >= DFL_MAX_BITS * DFL_ROW, "dynamic row scratch: 15 bits per byte");
static_assert(32 * (DFL_ROW_WORDS - 1) >= 9 * DFL_ROW, "fixed row scratch: 9 bits per byte");

// DflArgs.fmt: the samples of the written tile.  DFL_FMT_F32: float32 under
// predictor 3 (above).  DFL_FMT_U16: scaled 16-bit integers under predictor 2
// (TIFF 6.0 §14): the float sample is quantised (dfl_quantise) in the row
// load, the row's samples are differenced as 16-bit little-endian words
// (d[0] = q[0], d[c] = q[c] - q[c - 1] mod 65536, columns past the raster 0)
// and the 512 bytes (low byte of d[c], then its high byte) go to the row
// tokeniser as they are.  Everything that follows the row length -- the Adler
// partials, the raw size, the per-tile bound, the row scratch -- is below.
constexpr int DFL_FMT_F32 = 0, DFL_FMT_U16 = 1;
constexpr uint32_t DFL_U16_NODATA = 65535u, DFL_U16_MAX = 65534u;
constexpr int DFL_ROW16 = DFL_TILE * 2;
constexpr int64_t DFL_RAW16 = (int64_t)DFL_TILE * DFL_ROW16;   // 131072 bytes per tile
constexpr int64_t DFL_BOUND16 = ((2 + (19 + 9 * DFL_RAW16 + 14) / 8 + 4) + 15) / 16 * 16;
constexpr int DFL_ROW_WORDS16 = (9 * DFL_ROW16 + 31) / 32 + 1;
constexpr int DFL_ROW_WORDS16_DYN = (DFL_MAX_BITS * DFL_ROW16 + 31) / 32 + 1;
static_assert(32 * (DFL_ROW_WORDS16_DYN - 1) >= DFL_MAX_BITS * DFL_ROW16, "dynamic row scratch: 15 bits per byte");
static_assert(32 * (DFL_ROW_WORDS16 - 1) >= 9 * DFL_ROW16, "fixed row scratch: 9 bits per byte");
KF_HD constexpr int dfl_row_len(int fmt) { return fmt == DFL_FMT_U16 ? DFL_ROW16 : DFL_ROW; }
KF_HD constexpr int64_t dfl_raw(int fmt) { return fmt == DFL_FMT_U16 ? DFL_RAW16 : DFL_RAW; }
KF_HD constexpr int64_t dfl_bound(int fmt) { return fmt == DFL_FMT_U16 ? DFL_BOUND16 : DFL_BOUND; }
KF_HD constexpr int dfl_row_words(int fmt, bool dyn) {
  return fmt == DFL_FMT_U16 ? (dyn ? DFL_ROW_WORDS16_DYN : DFL_ROW_WORDS16) : (dyn ? DFL_ROW_WORDS_DYN : DFL_ROW_WORDS);
}

// The 16-bit sample of v for a raster with range [lo, hi]: a = 65534 / (hi - lo)
// and b = -lo * 65534 / (hi - lo), each formed in float64 and rounded once to
// float32 by the caller.  NaN is the nodata value 65535; everything else is
// clamp(rint(fma(v, a, b)), 0, 65534), +-inf included.  The fma is explicit, so
// no contraction setting decides a bit and the device and the host agree.  A
// sample whose rounded value falls outside [0, 65534] is saturated: ++sat.
KF_HD uint32_t dfl_quantise(float v, float a, float b, uint32_t& sat) {
  if (v != v) return DFL_U16_NODATA;
  const float t = __builtin_rintf(__builtin_fmaf(v, a, b));
  if (t < 0.f) {
    ++sat;
    return 0u;
  }
  if (t > (float)DFL_U16_MAX) {
    ++sat;
    return DFL_U16_MAX;
  }
  return (uint32_t)t;
}

KF_HD uint32_t dfl_rev(uint32_t code, int len) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_bitreverse32(code) >> (32 - len);
#else
  uint32_t r = 0;
  for (int i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
  return r;
#endif
}

// fixed-Huffman literal: (bits LSB-first, length)
KF_HD void dfl_lit(uint32_t v, uint32_t& bits, int& len) {
  if (v < 144u) {
    len = 8;
    bits = dfl_rev(0x30u + v, 8);
  } else {
    len = 9;
    bits = dfl_rev(0x190u + (v - 144u), 9);
  }
}

// length symbol (257..285) of a match of length L with its extra bits
KF_HD void dfl_len_code(int L, int& code, int& e, int& ev) {
  e = 0;
  ev = 0;
  if (L == 258) {
    code = 285;
  } else if (L <= 10) {
    code = 254 + L;
  } else {
    const int n = L - 3;
    int lg = 0;
    while ((n >> (lg + 1)) != 0) ++lg;        // floor(log2 n), n in [8, 254]
    e = lg - 2;
    code = 261 + 4 * e + (n >> e) - 4;
    ev = n & ((1 << e) - 1);
  }
}

// run-length match of length L (3..258) at distance 1: length code + extra
// bits + the 5-bit distance code 0, as one LSB-first bit string
KF_HD void dfl_match(int L, uint32_t& bits, int& len) {
  int code, e, ev;
  dfl_len_code(L, code, e, ev);
  uint32_t c;
  int cl;
  if (code < 280) {
    c = dfl_rev((uint32_t)(code - 256), 7);
    cl = 7;
  } else {
    c = dfl_rev(0xC0u + (uint32_t)(code - 280), 8);
    cl = 8;
  }
  bits = c | ((uint32_t)ev << cl);   // distance code 0 (5 zero bits) follows
  len = cl + e + 5;
}

// byte i of a predicted row (before differencing) from the row's samples
// (float bits; samples past the raster are 0): plane i / 256 is the sample's
// byte 3 - i / 256 (most significant first).  DFL_FMT_U16: row(i) is byte i of
// the row's 16-bit differences, which the caller forms in one pass over the columns
template <int FMT = DFL_FMT_F32, typename ROW>
KF_HD uint32_t dfl_row_byte(ROW&& row, int i) {
  if constexpr (FMT == DFL_FMT_U16) {
    return row(i);
  } else {
    const int k = i >> 8, c = i & 255;
    return (row(c) >> (8 * (3 - k))) & 0xFFu;
  }
}

// Tokenises one tile row: TOK(v, L) receives the tokens in order, a literal
// byte v (L = 0) or a distance-1 match of length L (3..258; v is the repeated
// byte).  Also returns the row's Adler-32 partial sums over its predicted bytes
// d: s1 = sum d, s2 = sum (rest - i) d with rest = bytes from the row's start
// to the end of the tile.  FMT: the row's length and whether its bytes are
// differenced here (float32, predictor 3) or arrive differenced (16-bit).
template <int FMT = DFL_FMT_F32, typename ROW, typename TOK>
KF_HD void dfl_tokenise_row(ROW&& row, int64_t rest, TOK&& tok, uint64_t& s1, uint64_t& s2) {
  uint32_t prev = dfl_row_byte<FMT>(row, 0);
  uint32_t last = prev;           // the last byte of the output so far (d)
  tok(last, 0);
  s1 = last;
  s2 = (uint64_t)rest * last;
  int run = 0;                    // bytes equal to `last` not yet emitted
  auto flush = [&]() {
    if (run >= 3) {
      tok(last, run);
    } else {
      for (int j = 0; j < run; ++j) tok(last, 0);
    }
    run = 0;
  };
  for (int i = 1; i < dfl_row_len(FMT); ++i) {
    const uint32_t r = dfl_row_byte<FMT>(row, i);
    const uint32_t d = FMT == DFL_FMT_U16 ? r : (r - prev) & 0xFFu;
    prev = r;
    s1 += d;
    s2 += (uint64_t)(rest - i) * d;
    if (d == last && run < 258) {
      ++run;
      continue;
    }
    flush();
    if (d == last) {              // a full 258 run ended: the next run repeats it
      run = 1;
      continue;
    }
    tok(d, 0);
    last = d;
  }
  flush();
}

// Encodes one tile row with the fixed Huffman codes: SINK(bits, len) receives
// the LSB-first bit strings in order (Adler partials as dfl_tokenise_row)
template <int FMT = DFL_FMT_F32, typename ROW, typename SINK>
KF_HD void dfl_encode_row(ROW&& row, int64_t rest, SINK&& sink, uint64_t& s1, uint64_t& s2) {
  dfl_tokenise_row<FMT>(row, rest, [&](uint32_t v, int L) {
    uint32_t b;
    int l;
    if (L) dfl_match(L, b, l);
    else dfl_lit(v, b, l);
    sink(b, l);
  }, s1, s2);
}

// Adler-32 from the tile's summed partials (n bytes)
KF_HD uint32_t dfl_adler(uint64_t s1, uint64_t s2, int64_t n) {
  const uint32_t a = (uint32_t)((1u + s1) % DFL_ADLER_MOD);
  const uint32_t b = (uint32_t)(((uint64_t)n + s2) % DFL_ADLER_MOD);
  return (b << 16) | a;
}

// ---------------------------------------------------------------- dynamic mode
// The block's code table: what the encode pass and the header writer read.
// Fixed fallback: the fixed codes, dist_len = 5, dynamic = 0.
struct DflTable {
  uint16_t code[DFL_NSYM];      // literal/length codes, bit-reversed (LSB-first)
  uint8_t len[DFL_NSYM];
  uint16_t cl_code[DFL_NCL];    // code-length code (dynamic block header)
  uint8_t cl_len[DFL_NCL];
  uint8_t dist_len;             // bits of the one distance code used (code 0): 1 dynamic, 5 fixed
  uint8_t dynamic;              // BTYPE 10 (1) or 01 (0)
  uint8_t hclen;                // code-length code lengths sent (4..19)
  uint16_t nlit;                // literal/length code lengths sent (257..286)
  uint32_t head_bits;           // BFINAL + BTYPE + the dynamic header: bits before the first token
  uint64_t block_bits;          // head_bits + tokens + end of block
};

// Work space of the table builder (LDS on the device, one lane runs it)
struct DflWork {
  uint32_t w[2 * DFL_NSYM];         // node weights, then node depths
  uint16_t parent[2 * DFL_NSYM];
  uint16_t sorted[DFL_NSYM];        // used symbols ascending by (frequency, index)
  uint32_t clfreq[DFL_NCL];
  uint32_t cnt[DFL_MAX_BITS + 1];   // codes per length; next canonical code per length
};

// position of symbol i among the used symbols (freq > 0) of freq[0..nsym) in
// ascending (frequency, index) order; -1 for an unused symbol
KF_HD int dfl_rank(const uint32_t* freq, int nsym, int i) {
  const uint32_t f = freq[i];
  if (f == 0) return -1;
  int rank = 0;
  for (int j = 0; j < nsym; ++j) {
    const uint32_t g = freq[j];
    rank += (g != 0 && (g < f || (g == f && j < i))) ? 1 : 0;
  }
  return rank;
}

// Code lengths (<= maxlen, Kraft sum exactly 1) of the n used symbols listed
// in k.sorted; lens[] is zero on entry.  One used symbol gets length 1 and so
// does one unused symbol (0, or 1 if symbol 0 is the used one): a complete code.
KF_HD void dfl_limited_lengths(const uint32_t* freq, int n, int maxlen, uint8_t* lens, DflWork& k) {
  const uint16_t* sorted = k.sorted;
  if (n == 1) {
    lens[sorted[0]] = 1;
    lens[sorted[0] == 0 ? 1 : 0] = 1;
    return;
  }
  uint32_t* w = k.w;
  uint16_t* par = k.parent;
  for (int i = 0; i < n; ++i) w[i] = freq[sorted[i]];
  // two-queue merge: leaves [0, n) in sorted order, internal nodes [n, 2n - 1)
  // in creation order (their weights never decrease); a leaf wins a tie
  int i = 0, j = n;
  for (int m = n; m < 2 * n - 1; ++m) {
    uint32_t s = 0;
    for (int t = 0; t < 2; ++t) {
      int a;
      if (i < n && (j >= m || w[i] <= w[j])) a = i++;
      else a = j++;
      s += w[a];
      par[a] = (uint16_t)m;
    }
    w[m] = s;
  }
  w[2 * n - 2] = 0;                                     // depths, root first
  for (int m = 2 * n - 3; m >= 0; --m) w[m] = w[par[m]] + 1u;
  uint32_t* cnt = k.cnt;
  for (int d = 0; d <= maxlen; ++d) cnt[d] = 0;
  for (int m = 0; m < n; ++m) ++cnt[w[m] < (uint32_t)maxlen ? w[m] : (uint32_t)maxlen];
  uint32_t total = 0;
  for (int d = 1; d <= maxlen; ++d) total += cnt[d] << (maxlen - d);
  while (total != (1u << maxlen)) {                    // over-subscribed by the folded depths
    --cnt[maxlen];
    for (int d = maxlen - 1; d > 0; --d) {
      if (cnt[d]) {
        --cnt[d];
        cnt[d + 1] += 2;
        break;
      }
    }
    --total;
  }
  int q = n;
  for (int d = 1; d <= maxlen; ++d)
    for (uint32_t l = cnt[d]; l > 0; --l) lens[sorted[--q]] = (uint8_t)d;
}

// canonical codes (RFC 1951 §3.2.2) from the lengths, bit-reversed
KF_HD void dfl_canonical(const uint8_t* lens, int nsym, int maxlen, uint16_t* code, DflWork& k) {
  uint32_t* next = k.cnt;
  for (int d = 0; d <= maxlen; ++d) next[d] = 0;
  for (int s = 0; s < nsym; ++s) ++next[lens[s]];
  uint32_t c = 0, prev = 0;
  next[0] = 0;
  for (int d = 1; d <= maxlen; ++d) {
    c = (c + prev) << 1;
    prev = next[d];
    next[d] = c;
  }
  for (int s = 0; s < nsym; ++s) {
    const int l = lens[s];
    code[s] = l ? (uint16_t)dfl_rev(next[l]++, l) : (uint16_t)0;
  }
}

// extra bits of length symbol s (257..285)
KF_HD int dfl_len_extra(int s) { return (s >= 265 && s < 285) ? (s - 261) >> 2 : 0; }

// The run-length coding of a sequence of n code lengths at(i): EMIT(symbol,
// extra bits, extra value) per code-length symbol, in order
template <typename AT, typename EMIT>
KF_HD void dfl_cl_tokens(AT&& at, int n, EMIT&& emit) {
  int i = 0;
  while (i < n) {
    const int v = at(i);
    int r = 1;
    while (i + r < n && at(i + r) == v) ++r;
    i += r;
    if (v == 0) {
      while (r >= 11) {
        const int m = r < 138 ? r : 138;
        emit(18, 7, m - 11);
        r -= m;
      }
      if (r >= 3) {
        emit(17, 3, r - 3);
        r = 0;
      }
      for (; r > 0; --r) emit(0, 0, 0);
    } else {
      emit(v, 0, 0);
      --r;
      while (r >= 3) {
        const int m = r < 6 ? r : 6;
        emit(16, 2, m - 3);
        r -= m;
      }
      for (; r > 0; --r) emit(v, 0, 0);
    }
  }
}

// order in which the code-length code's own lengths are sent (RFC 1951 §3.2.7)
KF_HD int dfl_cl_order(int i) {
  // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, 5 bits each
  const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 |
                      6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
  const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
  return (int)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31u);
}

// bits of the tokens and the end-of-block code of the fixed block + its 3 header bits
KF_HD uint64_t dfl_fixed_bits(const uint32_t* freq) {
  uint64_t bits = 3;
  for (int s = 0; s < DFL_NSYM; ++s) {
    const int l = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
    bits += (uint64_t)freq[s] * (uint64_t)(l + (s > 256 ? dfl_len_extra(s) + 5 : 0));
  }
  return bits;
}

// the fixed codes as a table (the dynamic mode's fallback block)
KF_HD void dfl_fixed_table(const uint32_t* freq, DflTable& t) {
  for (int s = 0; s < DFL_NSYM; ++s) {
    if (s < 144) {
      t.len[s] = 8;
      t.code[s] = (uint16_t)dfl_rev(0x30u + s, 8);
    } else if (s < 256) {
      t.len[s] = 9;
      t.code[s] = (uint16_t)dfl_rev(0x190u + (s - 144), 9);
    } else if (s < 280) {
      t.len[s] = 7;
      t.code[s] = (uint16_t)dfl_rev((uint32_t)(s - 256), 7);
    } else {
      t.len[s] = 8;
      t.code[s] = (uint16_t)dfl_rev(0xC0u + (uint32_t)(s - 280), 8);
    }
  }
  t.dist_len = 5;
  t.dynamic = 0;
  t.hclen = 0;
  t.nlit = 0;
  t.head_bits = 3;
  t.block_bits = dfl_fixed_bits(freq);
}

// The dynamic block's table from the tile's histogram freq[0..DFL_NSYM)
// (freq[256] = 1: the end-of-block code) with its n used symbols sorted in
// k.sorted (dfl_rank); fills t and returns the block's exact size in bits.
KF_HD uint64_t dfl_dynamic_table(const uint32_t* freq, int n, DflTable& t, DflWork& k) {
  for (int s = 0; s < DFL_NSYM; ++s) t.len[s] = 0;
  dfl_limited_lengths(freq, n, DFL_MAX_BITS, t.len, k);
  dfl_canonical(t.len, DFL_NSYM, DFL_MAX_BITS, t.code, k);
  int nlit = DFL_NSYM;
  while (nlit > 257 && t.len[nlit - 1] == 0) --nlit;
  t.nlit = (uint16_t)nlit;
  t.dist_len = 1;
  t.dynamic = 1;
  // the code-length code over the run-length coded lengths (+ the one distance length)
  auto at = [&](int i) -> int { return i < nlit ? (int)t.len[i] : 1; };
  for (int s = 0; s < DFL_NCL; ++s) {
    k.clfreq[s] = 0;
    t.cl_len[s] = 0;
  }
  uint32_t extra = 0;
  dfl_cl_tokens(at, nlit + 1, [&](int sym, int e, int) {
    ++k.clfreq[sym];
    extra += (uint32_t)e;
  });
  int ncl = 0;
  for (int s = 0; s < DFL_NCL; ++s) {
    const int r = dfl_rank(k.clfreq, DFL_NCL, s);
    if (r >= 0) {
      k.sorted[r] = (uint16_t)s;
      ++ncl;
    }
  }
  dfl_limited_lengths(k.clfreq, ncl, DFL_MAX_CL_BITS, t.cl_len, k);
  dfl_canonical(t.cl_len, DFL_NCL, DFL_MAX_CL_BITS, t.cl_code, k);
  int hclen = DFL_NCL;
  while (hclen > 4 && t.cl_len[dfl_cl_order(hclen - 1)] == 0) --hclen;
  t.hclen = (uint8_t)hclen;
  uint32_t head = 3 + 5 + 5 + 4 + 3 * (uint32_t)hclen + extra;
  for (int s = 0; s < DFL_NCL; ++s) head += k.clfreq[s] * t.cl_len[s];
  t.head_bits = head;
  uint64_t bits = head;
  for (int s = 0; s < DFL_NSYM; ++s)
    bits += (uint64_t)freq[s] * (uint64_t)(t.len[s] + (s > 256 ? dfl_len_extra(s) + 1 : 0));
  t.block_bits = bits;
  return bits;
}

// The per-tile choice: the dynamic block when it is strictly smaller than the
// fixed one, else the fixed block (force_fixed: always the fixed block)
KF_HD void dfl_choose_table(const uint32_t* freq, int n, bool force_fixed, DflTable& t, DflWork& k) {
  if (!force_fixed && dfl_dynamic_table(freq, n, t, k) < dfl_fixed_bits(freq)) return;
  dfl_fixed_table(freq, t);
}

// BFINAL, BTYPE and, for a dynamic block, the code tables (t.head_bits bits)
template <typename SINK>
KF_HD void dfl_write_block_header(const DflTable& t, SINK&& sink) {
  sink(1u, 1);                                  // BFINAL
  if (!t.dynamic) {
    sink(1u, 2);                                // BTYPE 01
    return;
  }
  sink(2u, 2);                                  // BTYPE 10
  const int nlit = t.nlit;
  sink((uint32_t)(nlit - 257), 5);              // HLIT
  sink(0u, 5);                                  // HDIST: one distance code
  sink((uint32_t)(t.hclen - 4), 4);             // HCLEN
  for (int i = 0; i < t.hclen; ++i) sink(t.cl_len[dfl_cl_order(i)], 3);
  auto at = [&](int i) -> int { return i < nlit ? (int)t.len[i] : 1; };
  dfl_cl_tokens(at, nlit + 1, [&](int sym, int e, int ev) {
    const int l = t.cl_len[sym];
    sink((uint32_t)t.cl_code[sym] | ((uint32_t)ev << l), l + e);
  });
}

// one token with the block's table: (bits LSB-first, length <= 25)
KF_HD void dfl_table_token(const DflTable& t, uint32_t v, int L, uint32_t& bits, int& len) {
  if (L == 0) {
    bits = t.code[v];
    len = t.len[v];
    return;
  }
  int code, e, ev;
  dfl_len_code(L, code, e, ev);
  const int cl = t.len[code];
  bits = (uint32_t)t.code[code] | ((uint32_t)ev << cl);   // the distance code 0 follows: zero bits
  len = cl + e + t.dist_len;
}

// histogram bin of a token
KF_HD int dfl_token_symbol(uint32_t v, int L) {
  if (L == 0) return (int)v;
  int code, e, ev;
  dfl_len_code(L, code, e, ev);
  return code;
}

}  // namespace kf
