// kf_inflate.h — GeoTIFF tile decoding on the device: one zlib stream (RFC
// 1950 / 1951) with a known output size per tile, the mirror image of
// kf_deflate.h.  Integer code only; the gfx950 kernel (kf_inflate.hip) and the
// host runner (kf_host.cpp) run this source, so their bytes and statuses are
// the same.
//
// The decoder is a resumable state machine (inf_step): Huffman decoding is
// serial per stream, so ONE lane runs it and appends tokens -- a literal byte
// or a (length, distance) match -- to a small queue; when the queue is full,
// a stored block's payload is due, or the stream ends, it returns and the
// caller drains the queue in order (the device: the whole wave, lane-parallel
// over the bytes of a match; the host: serially).  A stored block's payload is
// never queued: inf_step leaves its byte range in (sto_off, sto_len) and the
// caller copies it.
//
// Handled: the zlib header (CM = 8, CINFO <= 7, FCHECK, FDICT = 0), any number
// of blocks, stored blocks (LEN / NLEN), fixed and dynamic Huffman blocks
// (HLIT / HDIST / HCLEN, code-length symbols 16 / 17 / 18 with repeats that
// cross the literal / distance boundary), lengths 3..258 and distances
// 1..32768 with all extra bits, and the Adler-32 trailer.  Code sets follow
// zlib's rules: an over-subscribed set is rejected, an incomplete one too,
// except a single code of length 1 (dfl_dynamic_table sends such a distance
// code) and an empty set (every use of it is then an invalid symbol).
//
// Safety: every input read is bounded by the stream's byte count (bits past
// the end read as zero and taking them is INF_TRUNCATED); a token is queued
// only after its output range [produced, produced + length) has been checked
// against the raw size and its distance against `produced`; every loop
// iteration consumes input bits or returns.  Malformed input therefore ends in
// a status, never in an out-of-range access or a spin.
#pragma once
#include <stdint.h>
#include "kf_core.h"
#include "kf_deflate.h"
#include "kf_launch.h"

namespace kf {

constexpr int INF_QUEUE = 64;          // tokens per drain: one per lane of a wave
constexpr int INF_WINDOW = 32768;      // DEFLATE's largest distance
constexpr int INF_LIT_BITS = 9;        // first-level lookup, literal / length code
constexpr int INF_DIST_BITS = 6;       // first-level lookup, distance code
constexpr int INF_NLIT = 288, INF_NDIST = 32;
// phases of a stream
constexpr int INF_P_HEADER = 0, INF_P_BLOCK = 1, INF_P_CODES = 2, INF_P_TRAILER = 3, INF_P_DONE = 4;

// token: a literal byte (bit 31 clear), or bit 31 | (distance - 1) << 8 | (length - 3)
KF_HD uint32_t inf_tok_match(uint32_t len, uint32_t dist) { return 0x80000000u | ((dist - 1u) << 8) | (len - 3u); }
KF_HD bool inf_tok_is_match(uint32_t t) { return (t >> 31) != 0; }
KF_HD uint32_t inf_tok_len(uint32_t t) { return (t & 0xFFu) + 3u; }
KF_HD uint32_t inf_tok_dist(uint32_t t) { return ((t >> 8) & 0x7FFFu) + 1u; }

// Decode tables of the current block (LDS on the device: one set per wave).
// A first-level entry is symbol | length << 9 (0: no code of <= the lookup
// width starts with these bits); longer codes take the canonical count / offset
// walk over cnt[] / sym[] (symbols sorted by code length, then by index).
struct InfTables {
  uint16_t lfast[1 << INF_LIT_BITS];
  uint16_t dfast[1 << INF_DIST_BITS];
  uint16_t lcnt[16], dcnt[16], ccnt[16];
  uint16_t lsym[INF_NLIT], dsym[INF_NDIST], csym[DFL_NCL];
  uint16_t offs[16];                        // inf_build: first slot of each length in sym[]
  uint8_t lens[INF_NLIT + INF_NDIST];       // code lengths as they are read (fixed block: all 320)
};

struct InfState {
  const uint8_t* in;      // the stream
  uint32_t n;             // its byte count
  uint32_t pos;           // next byte to load into the bit buffer
  uint64_t hold;          // bit buffer, LSB first; bits past the stream are zero
  int32_t cnt;            // valid bits in hold
  int32_t phase, final, status;
  uint32_t produced;      // output bytes so far, queued tokens included
  uint32_t raw;           // the tile's raw size: the output must be exactly this
  uint32_t sto_off, sto_len;   // stored payload the caller has to copy: in[sto_off, sto_off + sto_len)
  uint32_t adler;         // the trailer's Adler-32 (phase INF_P_DONE)
};

KF_HD void inf_init(InfState& s, const uint8_t* in, uint32_t n, uint32_t raw) {
  s.in = in;
  s.n = n;
  s.pos = 0;
  s.hold = 0;
  s.cnt = 0;
  s.phase = INF_P_HEADER;
  s.final = 0;
  s.status = INF_OK;
  s.produced = 0;
  s.raw = raw;
  s.sto_off = s.sto_len = 0;
  s.adler = 0;
}

// at least 33 valid bits afterwards, unless the stream ends before
KF_HD void inf_refill(InfState& s) {
  if (s.cnt > 32) return;
  if (s.n - s.pos >= 4u) {
    KF_DCHECK(s.pos + 4u <= s.n);
    uint32_t w;
    __builtin_memcpy(&w, s.in + s.pos, 4);
    s.hold |= (uint64_t)w << s.cnt;
    s.pos += 4;
    s.cnt += 32;
    return;
  }
  while (s.cnt <= 56 && s.pos < s.n) {
    KF_DCHECK(s.pos < s.n);
    s.hold |= (uint64_t)s.in[s.pos++] << s.cnt;
    s.cnt += 8;
  }
}

// k <= 16 bits; past the end: INF_TRUNCATED and 0
KF_HD uint32_t inf_take(InfState& s, int k) {
  if (k > s.cnt) {
    s.status = INF_TRUNCATED;
    return 0;
  }
  const uint32_t v = (uint32_t)s.hold & ((1u << k) - 1u);
  s.hold >>= k;
  s.cnt -= k;
  return v;
}

// One symbol of a code (refill first: a code has <= 15 bits).  -1 with the
// status set: no code starts with the next bits (INF_BAD_SYMBOL), or the
// stream ends inside the code (INF_TRUNCATED).
KF_HD int inf_symbol(InfState& s, const uint16_t* fast, int fbits, const uint16_t* cnt, const uint16_t* sym, int nsym) {
  if (fbits) {
    const uint32_t e = fast[(uint32_t)s.hold & ((1u << fbits) - 1u)];
    if (e) {
      const int l = (int)(e >> 9);
      if (l > s.cnt) {
        s.status = INF_TRUNCATED;
        return -1;
      }
      s.hold >>= l;
      s.cnt -= l;
      return (int)(e & 511u);
    }
  }
  int code = 0, first = 0, index = 0;
  uint32_t h = (uint32_t)s.hold;
  for (int len = 1; len <= DFL_MAX_BITS; ++len) {
    code |= (int)(h & 1u);
    h >>= 1;
    const int c = cnt[len];
    if (code - c < first) {
      if (len > s.cnt) {
        s.status = INF_TRUNCATED;
        return -1;
      }
      s.hold >>= len;
      s.cnt -= len;
      KF_DCHECK(index + (code - first) >= 0 && index + (code - first) < nsym);
      return sym[index + (code - first)];
    }
    index += c;
    first += c;
    first <<= 1;
    code <<= 1;
  }
  (void)nsym;
  s.status = s.cnt < DFL_MAX_BITS ? INF_TRUNCATED : INF_BAD_SYMBOL;
  return -1;
}

// Decode tables from n code lengths (0..15).  false: the set is
// over-subscribed, or incomplete and neither empty nor (allow_single) one code
// of length 1.
KF_HD bool inf_build(const uint8_t* lens, int n, uint16_t* cnt, uint16_t* sym, uint16_t* fast, int fbits,
                     bool allow_single, uint16_t* offs) {
  for (int l = 0; l <= DFL_MAX_BITS; ++l) cnt[l] = 0;
  for (int i = 0; i < n; ++i) {
    KF_DCHECK(lens[i] <= DFL_MAX_BITS);
    ++cnt[lens[i]];
  }
  const int ncodes = n - cnt[0];
  cnt[0] = 0;
  int left = 1;
  for (int l = 1; l <= DFL_MAX_BITS; ++l) {
    left <<= 1;
    left -= cnt[l];
    if (left < 0) return false;
  }
  if (left > 0 && ncodes != 0 && !(allow_single && ncodes == 1 && cnt[1] == 1)) return false;
  offs[1] = 0;
  for (int l = 1; l < DFL_MAX_BITS; ++l) offs[l + 1] = (uint16_t)(offs[l] + cnt[l]);
  for (int i = 0; i < n; ++i)
    if (lens[i]) {
      KF_DCHECK(offs[lens[i]] < n);
      sym[offs[lens[i]]++] = (uint16_t)i;
    }
  if (fbits) {
    for (int i = 0; i < (1 << fbits); ++i) fast[i] = 0;
    // canonical codes in sym[] order: consecutive within a length, doubled between lengths
    uint32_t code = 0;
    int idx = 0;
    for (int l = 1; l <= fbits; ++l) {
      for (int k = 0; k < cnt[l]; ++k) {
        const uint32_t e = (uint32_t)sym[idx++] | ((uint32_t)l << 9);
        for (uint32_t j = dfl_rev(code, l); j < (1u << fbits); j += 1u << l) fast[j] = (uint16_t)e;
        ++code;
      }
      code <<= 1;
    }
  }
  return true;
}

// length of symbol s (257..285) without its extra bits, and their count
KF_HD uint32_t inf_len_base(int s, int& extra) {
  if (s < 265) {
    extra = 0;
    return (uint32_t)(s - 254);
  }
  if (s == 285) {
    extra = 0;
    return 258u;
  }
  extra = (s - 261) >> 2;
  return 3u + ((4u + (uint32_t)((s - 261) & 3)) << extra);
}

// distance of symbol d (0..29) without its extra bits, and their count
KF_HD uint32_t inf_dist_base(int d, int& extra) {
  if (d < 4) {
    extra = 0;
    return (uint32_t)(d + 1);
  }
  extra = (d >> 1) - 1;
  return 1u + ((2u + (uint32_t)(d & 1)) << extra);
}

KF_HD void inf_fail(InfState& s, int status) {
  if (s.status == INF_OK) s.status = status;
}

// tables of a fixed block (RFC 1951 §3.2.6): symbols 286 / 287 and distances
// 30 / 31 take part in the codes and are invalid when they occur
KF_HD void inf_fixed_tables(InfTables& t) {
  for (int i = 0; i < INF_NLIT; ++i) t.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
  for (int i = 0; i < INF_NDIST; ++i) t.lens[INF_NLIT + i] = 5;
  inf_build(t.lens, INF_NLIT, t.lcnt, t.lsym, t.lfast, INF_LIT_BITS, false, t.offs);
  inf_build(t.lens + INF_NLIT, INF_NDIST, t.dcnt, t.dsym, t.dfast, INF_DIST_BITS, false, t.offs);
}

// the code tables of a dynamic block (RFC 1951 §3.2.7); false with the status set
KF_HD bool inf_dynamic_tables(InfState& s, InfTables& t) {
  inf_refill(s);
  const int hlit = (int)inf_take(s, 5) + 257, hdist = (int)inf_take(s, 5) + 1, hclen = (int)inf_take(s, 4) + 4;
  if (s.status != INF_OK) return false;
  if (hlit > 286 || hdist > 30) {
    inf_fail(s, INF_BAD_CODE);
    return false;
  }
  for (int i = 0; i < DFL_NCL; ++i) t.lens[i] = 0;
  for (int i = 0; i < hclen; ++i) {
    inf_refill(s);
    t.lens[dfl_cl_order(i)] = (uint8_t)inf_take(s, 3);
    if (s.status != INF_OK) return false;
  }
  if (!inf_build(t.lens, DFL_NCL, t.ccnt, t.csym, nullptr, 0, false, t.offs)) {
    inf_fail(s, INF_BAD_CODE);
    return false;
  }
  const int n = hlit + hdist;
  int i = 0;
  while (i < n) {                       // every iteration takes >= 1 bit or returns
    inf_refill(s);
    const int sym = inf_symbol(s, nullptr, 0, t.ccnt, t.csym, DFL_NCL);
    if (sym < 0) return false;
    if (sym < 16) {
      KF_DCHECK(i < INF_NLIT + INF_NDIST);
      t.lens[i++] = (uint8_t)sym;
      continue;
    }
    int rep, val = 0;
    if (sym == 16) {
      if (i == 0) {
        inf_fail(s, INF_BAD_CODE);
        return false;
      }
      val = t.lens[i - 1];
      rep = 3 + (int)inf_take(s, 2);
    } else if (sym == 17) {
      rep = 3 + (int)inf_take(s, 3);
    } else {
      rep = 11 + (int)inf_take(s, 7);
    }
    if (s.status != INF_OK) return false;
    if (i + rep > n) {
      inf_fail(s, INF_BAD_CODE);
      return false;
    }
    for (; rep > 0; --rep) {
      KF_DCHECK(i < INF_NLIT + INF_NDIST);
      t.lens[i++] = (uint8_t)val;
    }
  }
  if (t.lens[256] == 0 ||
      !inf_build(t.lens, hlit, t.lcnt, t.lsym, t.lfast, INF_LIT_BITS, true, t.offs) ||
      !inf_build(t.lens + hlit, hdist, t.dcnt, t.dsym, t.dfast, INF_DIST_BITS, true, t.offs)) {
    inf_fail(s, INF_BAD_CODE);
    return false;
  }
  return true;
}

// The caller has copied the stored payload: continue behind it.
KF_HD void inf_stored_done(InfState& s) {
  s.pos = s.sto_off + s.sto_len;
  s.hold = 0;
  s.cnt = 0;
  s.produced += s.sto_len;
  s.sto_len = 0;
  s.phase = s.final ? INF_P_TRAILER : INF_P_BLOCK;
}

// Runs the stream until q[0..qcap) is full, a stored payload is due
// (s.sto_len > 0: drain the queue, copy in[sto_off, +sto_len) to the output,
// call again), the stream is complete (phase INF_P_DONE, s.adler set) or
// broken (s.status).  Returns the number of tokens queued.  Every call takes
// at least one bit from the stream or ends it.
KF_HD int inf_step(InfState& s, InfTables& t, uint32_t* q, int qcap) {
  int nq = 0;
  if (s.sto_len) inf_stored_done(s);
  for (;;) {
    if (s.status != INF_OK || s.phase == INF_P_DONE) return nq;
    if (s.phase == INF_P_HEADER) {
      inf_refill(s);
      const uint32_t cmf = inf_take(s, 8), flg = inf_take(s, 8);
      if (s.status != INF_OK) return nq;
      if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 0x20u)) {
        inf_fail(s, INF_BAD_HEADER);
        return nq;
      }
      s.phase = INF_P_BLOCK;
    } else if (s.phase == INF_P_BLOCK) {
      inf_refill(s);
      s.final = (int)inf_take(s, 1);
      const uint32_t type = inf_take(s, 2);
      if (s.status != INF_OK) return nq;
      if (type == 0) {
        inf_take(s, s.cnt & 7);         // to the byte boundary
        inf_refill(s);
        const uint32_t len = inf_take(s, 16), nlen = inf_take(s, 16);
        if (s.status != INF_OK) return nq;
        if (len != (~nlen & 0xFFFFu)) {
          inf_fail(s, INF_BAD_STORED);
          return nq;
        }
        KF_DCHECK((s.cnt & 7) == 0 && s.pos >= (uint32_t)(s.cnt >> 3));
        const uint32_t at = s.pos - (uint32_t)(s.cnt >> 3);    // the payload's first byte
        if (len > s.n - at) {
          inf_fail(s, INF_TRUNCATED);
          return nq;
        }
        if (len > s.raw - s.produced) {
          inf_fail(s, INF_OVERRUN);
          return nq;
        }
        s.sto_off = at;
        s.sto_len = len;
        if (len) return nq;             // the caller copies, the next call continues behind it
        inf_stored_done(s);             // an empty stored block (a flush)
      } else if (type == 1) {
        inf_fixed_tables(t);
        s.phase = INF_P_CODES;
      } else if (type == 2) {
        if (!inf_dynamic_tables(s, t)) return nq;
        s.phase = INF_P_CODES;
      } else {
        inf_fail(s, INF_BAD_BLOCK);
        return nq;
      }
    } else if (s.phase == INF_P_CODES) {
      while (nq < qcap) {               // every iteration takes >= 1 bit or returns
        inf_refill(s);
        const int sym = inf_symbol(s, t.lfast, INF_LIT_BITS, t.lcnt, t.lsym, INF_NLIT);
        if (sym < 0) return nq;
        if (sym < 256) {
          if (s.produced >= s.raw) {
            inf_fail(s, INF_OVERRUN);
            return nq;
          }
          q[nq++] = (uint32_t)sym;
          ++s.produced;
          continue;
        }
        if (sym == 256) {
          s.phase = s.final ? INF_P_TRAILER : INF_P_BLOCK;
          break;
        }
        if (sym >= 286) {
          inf_fail(s, INF_BAD_SYMBOL);
          return nq;
        }
        int e;
        uint32_t len = inf_len_base(sym, e);
        len += inf_take(s, e);
        inf_refill(s);
        const int ds = inf_symbol(s, t.dfast, INF_DIST_BITS, t.dcnt, t.dsym, INF_NDIST);
        if (ds < 0) return nq;
        if (ds >= 30) {
          inf_fail(s, INF_BAD_SYMBOL);
          return nq;
        }
        uint32_t dist = inf_dist_base(ds, e);
        dist += inf_take(s, e);
        if (s.status != INF_OK) return nq;
        KF_DCHECK(len >= 3 && len <= 258 && dist >= 1 && dist <= (uint32_t)INF_WINDOW);
        if (dist > s.produced) {
          inf_fail(s, INF_BAD_DISTANCE);
          return nq;
        }
        if (len > s.raw - s.produced) {
          inf_fail(s, INF_OVERRUN);
          return nq;
        }
        q[nq++] = inf_tok_match(len, dist);
        s.produced += len;
      }
      if (s.phase == INF_P_CODES) return nq;   // the queue is full
    } else {                            // INF_P_TRAILER
      if (s.produced != s.raw) {
        inf_fail(s, INF_SHORT);
        return nq;
      }
      inf_take(s, s.cnt & 7);
      inf_refill(s);
      uint32_t a = 0;
      for (int k = 0; k < 4; ++k) a = (a << 8) | inf_take(s, 8);   // big-endian
      if (s.status != INF_OK) return nq;
      s.adler = a;
      s.phase = INF_P_DONE;
    }
  }
}

// Adler-32 partial sums of byte b at output index i of n (dfl_adler combines them)
KF_HD void inf_adler_add(uint64_t& s1, uint64_t& s2, uint32_t b, uint32_t i, uint32_t n) {
  s1 += b;
  s2 += (uint64_t)(n - i) * b;
}

// The serial drain (host runner): tokens q[0..nq) into raw at pos
KF_HD void inf_drain_serial(const uint32_t* q, int nq, uint8_t* raw, uint32_t& pos, uint32_t n, uint64_t& s1,
                            uint64_t& s2) {
  for (int k = 0; k < nq; ++k) {
    const uint32_t tk = q[k];
    if (!inf_tok_is_match(tk)) {
      KF_DCHECK(pos < n);
      raw[pos] = (uint8_t)tk;
      inf_adler_add(s1, s2, tk & 0xFFu, pos, n);
      ++pos;
      continue;
    }
    const uint32_t len = inf_tok_len(tk), dist = inf_tok_dist(tk);
    KF_DCHECK(dist <= pos && len <= n - pos);
    for (uint32_t j = 0; j < len; ++j) {
      const uint32_t b = raw[pos - dist + (dist >= len ? j : j % dist)];
      raw[pos + j] = (uint8_t)b;
      inf_adler_add(s1, s2, b, pos + j, n);
    }
    pos += len;
  }
}

// scratch bytes per tile: the raw size the streams announce or the tile the
// placement reads, whichever is larger, in 16-byte units
KF_HD int64_t inf_scratch_stride(int64_t raw_bytes, int tile, int elem_bytes) {
  const int64_t t = (int64_t)tile * tile * elem_bytes;
  return ((raw_bytes > t ? raw_bytes : t) + 15) / 16 * 16;
}

KF_HD bool inf_args_ok(const InfArgs& a) {
  return a.ntiles > 0 && a.tile == DFL_TILE &&
         ((a.elem_bytes == 2 && (a.predictor == 1 || a.predictor == 2)) ||
          (a.elem_bytes == 4 && (a.predictor == 1 || a.predictor == 3))) &&
         a.raw_bytes > 0 && a.raw_bytes <= (int64_t)1 << 30 && a.comp_bytes >= 0 && a.r0 >= 0 && a.c0 >= 0 &&
         a.r0 < a.r1 && a.c0 < a.c1 && a.ld >= a.c1 - a.c0;
}

}  // namespace kf
