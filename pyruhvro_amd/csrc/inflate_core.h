// RFC 1951 raw deflate, written once for the device (inflate.hip) and for the host (tools/inflate_check.cpp): DESIGN.md 14,
// "Deflate blocks on the device".  No HIP include is needed on the host side; not one of the headers the specialised kernels
// include, so the kernel-cache key does not see this file.
//
// One call of inflate_stream walks ONE raw-deflate stream (one container block) from (ptr, len) into a Sink:
//   Sink::lit(byte)            one literal
//   Sink::copy(length, dist)   a match: `length` bytes from `dist` bytes back (dist <= produced() was checked)
//   Sink::stored(src, n)       n bytes of a stored block, straight from the input
//   Sink::produced()           bytes so far, in 64 bits
// each returning false when the sink will not take the bytes (an emit walk that disagrees with its size pass): the walk then
// stops with ST_INTERNAL and stores nothing more.  A size walk is the same function over a sink that only counts.
//
// Verdicts are zlib's (inflate.c / inftrees.c, 1.2.11 and later), because the host road is zlib and both roads must agree on
// what a valid stream is.  Where a stream is both damaged and cut short the verdict is the one zlib meets first in stream
// order: every check below stands where zlib's stands relative to the bits it needs (NEEDBITS before the test).
//
// On the device every lane of a wavefront runs this walk over the same input, so all state is wave-uniform by construction and
// the cooperative steps of a sink (the match copy, the flush) sit in uniform control flow.  Only the `writer` lane stores into
// the tables; RHI_SYNC() orders those stores before the other lanes' loads.
//
// TERMINATION.  Every loop either runs a constant number of times or consumes input, so a walk takes O(len) steps plus the
// bytes it produces, whatever the bytes are:
//   - the block loop consumes the 3 header bits per turn, or returns;
//   - the symbol loop calls decode() once per turn, which drops a code of 1 .. 15 bits or returns a verdict (the slow path's own
//     loop is bounded by 15 lengths); a length / distance pair adds at most 258 bytes of output per turn;
//   - the code-length loop drops one code of 1 .. 7 bits per turn (zlib's 1-bit "no code at all" entry included) or returns;
//     the run it writes is bounded by 138 and by HLIT + HDIST <= 316;
//   - the HCLEN loop runs 4 .. 19 times, build() loops over at most 288 symbols, 15 lengths and 1024 table entries;
//   - a stored block consumes its 32 header bits; its copy is bounded by 65,535 and by the input left;
//   - fill() pulls at most 8 bytes and never reads outside [ptr, ptr + len).
// Output is bounded by 258 bytes per input bit, and by max_out: a walk stops with ST_TOO_LARGE once it has produced that much.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RHI_HD __host__ __device__ __forceinline__
#else
#define RHI_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define RHI_SYNC() __syncthreads()      // (the workgroup is one wavefront: this is the fence, the barrier costs nothing)
#else
#define RHI_SYNC() ((void)0)
#endif

namespace rhi {

// rh_inflate_status.code (include/ruhvro_hip.h: RH_INFLATE_*)
enum : uint32_t { ST_OK = 0, ST_MALFORMED = 1, ST_TRUNCATED = 2, ST_TRAILING = 3, ST_TOO_LARGE = 4, ST_INTERNAL = 5 };

// rh_inflate_status.reason of ST_MALFORMED: one per rule (the texts: engine_container.cpp inflate_reason)
enum : uint32_t {
  R_NONE = 0,
  R_BLOCK_TYPE = 1,       // block type 3
  R_STORED_LEN = 2,       // stored LEN != ~NLEN
  R_TOO_MANY = 3,         // HLIT > 286 or HDIST > 30
  R_REPEAT = 4,           // a repeat with nothing to repeat, or one that runs past HLIT + HDIST
  R_NO_EOB = 5,           // no code for end-of-block
  R_OVERSUBSCRIBED = 6,   // detail: 0 the code-length code, 1 literal/length, 2 distance
  R_INCOMPLETE = 7,       // detail likewise
  R_NO_CODE = 8,          // a decoded symbol that has no code; detail: 1 literal/length, 2 distance
  R_LITLEN_286 = 9,       // literal/length symbol 286 or 287
  R_DIST_30 = 10,         // distance symbol 30 or 31
  R_TOO_FAR = 11,         // a distance further back than the bytes produced so far
  R_COUNT = 12
};

struct Status {
  uint32_t code, reason;
  uint64_t detail;
};
RHI_HD Status status(uint32_t code, uint32_t reason = R_NONE, uint64_t detail = 0) {
  Status s;
  s.code = code; s.reason = reason; s.detail = detail;
  return s;
}

// ---- the base / extra-bit tables of RFC 1951 3.2.5, as arithmetic (tools/inflate_check.cpp holds them as the RFC prints them
// and compares): length symbol 257 + s, s in 0 .. 28; distance symbol d in 0 .. 29
RHI_HD uint32_t len_extra(uint32_t s) { return s < 8 || s == 28 ? 0 : (s - 4) >> 2; }
RHI_HD uint32_t len_base(uint32_t s) { return s < 8 ? 3 + s : s == 28 ? 258 : 3 + ((4 + (s & 3)) << ((s - 4) >> 2)); }
RHI_HD uint32_t dist_extra(uint32_t d) { return d < 4 ? 0 : (d - 2) >> 1; }
RHI_HD uint32_t dist_base(uint32_t d) { return d < 4 ? 1 + d : 1 + ((2 + (d & 1)) << ((d - 2) >> 1)); }

// the permuted order of the code-length code's lengths, 5 bits each in two words
constexpr uint64_t clen_order_word(int from, int to) {
  const uint8_t o[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  uint64_t v = 0;
  for (int i = from; i < to; i++) v |= (uint64_t)o[i] << (5 * (i - from));
  return v;
}
constexpr uint64_t kClenOrderLo = clen_order_word(0, 12), kClenOrderHi = clen_order_word(12, 19);
RHI_HD uint32_t clen_order(uint32_t i) { return (uint32_t)((i < 12 ? kClenOrderLo >> (5 * i) : kClenOrderHi >> (5 * (i - 12))) & 31); }

// ---- bit reader over (p, len): LSB first, never reads outside [p, p + len) ----------------------------------------------------
struct Bits {
  const uint8_t* p;
  uint64_t len, pos;      // pos: bytes taken into hold
  uint64_t hold;          // the low `cnt` bits are the next bits of the stream; bits above them repeat what is at p[pos ..]
  uint32_t cnt;

  RHI_HD void init(const uint8_t* ptr, uint64_t n) { p = ptr; len = n; pos = 0; hold = 0; cnt = 0; }
  RHI_HD void fill() {
    if (len - pos >= 8) {
      uint64_t w;
      __builtin_memcpy(&w, p + pos, 8);      // (little-endian on both sides)
      hold |= w << cnt;
      pos += (63u - cnt) >> 3;
      cnt |= 56u;
    } else {
      while (cnt <= 56 && pos < len) { hold |= (uint64_t)p[pos] << cnt; pos++; cnt += 8; }
    }
  }
  RHI_HD bool need(uint32_t n) {      // n <= 32
    if (cnt < n) fill();
    return cnt >= n;
  }
  RHI_HD uint32_t peek(uint32_t n) const { return (uint32_t)(hold & ((1ull << n) - 1)); }
  RHI_HD void drop(uint32_t n) { hold >>= n; cnt -= n; }
  RHI_HD void to_byte() { drop(cnt & 7); }      // (cnt counts whole bytes above the stream's position)
  // the bytes in hold go back to the input: pos is the stream's position (call at a byte boundary)
  RHI_HD void rewind() { pos -= cnt >> 3; cnt = 0; hold = 0; }
  RHI_HD uint64_t bytes_used() const { return pos - (cnt >> 3); }      // up to and with the byte that holds the last bit taken
};

// ---- codes --------------------------------------------------------------------------------------------------------------------
constexpr int kLitBits = 10, kDistBits = 8, kClenBits = 7;      // lookup widths; every code-length code fits its own
constexpr uint16_t kNoSym = 0xFFF;                              // a code that stands for no symbol (zlib's op = 64 entries)
constexpr int D_TRUNCATED = -1, D_NO_CODE = -2;

// A canonical code: count[l] codes of l bits, their symbols in code order, and a lookup over the next W bits:
// (symbol << 4) | bits for a code of at most W bits, 0 for a longer one (the slow path finds it from count / symbol).
struct Tables {
  uint16_t lfast[1 << kLitBits], dfast[1 << kDistBits], cfast[1 << kClenBits];
  uint16_t lcount[16], dcount[16], ccount[16];
  uint16_t lsym[288], dsym[32], csym[19];
  uint8_t lens[320], clens[19];
  uint8_t fixed_ready;      // the l / d tables hold the fixed code
};

// zlib's inflate_table: 0, or R_OVERSUBSCRIBED / R_INCOMPLETE.  A code with no symbol at all is accepted (two 1-bit entries
// that stand for nothing); an incomplete code only as a single 1-bit code (never for the code-length code).
RHI_HD uint32_t build(const uint8_t* lens, uint32_t n, uint16_t* count, uint16_t* sym, uint16_t* fast, uint32_t W, bool is_clen, bool writer) {
  uint16_t cnt[16], offs[16];
  for (int l = 0; l < 16; l++) cnt[l] = 0;
  for (uint32_t i = 0; i < n; i++) cnt[lens[i] & 15]++;
  int max = 15;
  while (max > 0 && cnt[max] == 0) max--;
  int left = 1;
  for (int l = 1; l < 16 && max; l++) {
    left <<= 1;
    left -= cnt[l];
    if (left < 0) return R_OVERSUBSCRIBED;
  }
  if (max && left > 0 && (is_clen || max != 1)) return R_INCOMPLETE;
  if (writer) {
    for (int l = 0; l < 16; l++) count[l] = cnt[l];
    offs[1] = 0;
    for (int l = 1; l < 15; l++) offs[l + 1] = (uint16_t)(offs[l] + cnt[l]);
    for (uint32_t i = 0; i < n; i++)
      if (lens[i]) sym[offs[lens[i] & 15]++] = (uint16_t)i;
    // the lookup: nothing is a code until a symbol claims it; with no code at all, or one 1-bit code, the rest are 1-bit holes
    const uint16_t hole = max <= 1 ? (uint16_t)((kNoSym << 4) | 1) : (uint16_t)0;
    for (uint32_t j = 0; j < (1u << W); j++) fast[j] = hole;
    uint32_t code = 0, at = 0;
    for (uint32_t l = 1; l <= W; l++) {
      for (uint32_t k = 0; k < cnt[l]; k++, code++, at++) {
        uint32_t rev = 0;
        for (uint32_t b = 0; b < l; b++) rev |= ((code >> b) & 1u) << (l - 1 - b);
        const uint16_t e = (uint16_t)((sym[at] << 4) | l);
        for (uint32_t j = rev; j < (1u << W); j += 1u << l) fast[j] = e;
      }
      code <<= 1;
    }
  }
  return 0;
}

// The next symbol, or D_TRUNCATED (its code needs more bits than the input has), or D_NO_CODE.  Drops the code's bits.
RHI_HD int decode(Bits& B, const uint16_t* count, const uint16_t* sym, const uint16_t* fast, uint32_t W) {
  if (B.cnt < 15) B.fill();
  const uint32_t e = fast[B.hold & ((1u << W) - 1)];
  const uint32_t l = e & 15;
  if (l) {      // (a code shorter than W is found with fewer than W bits left: the bits above cnt are zero or the stream's own)
    if (l > B.cnt) return D_TRUNCATED;
    B.drop(l);
    return (e >> 4) == kNoSym ? D_NO_CODE : (int)(e >> 4);
  }
  // longer than W: canonical decode, one length at a time
  uint32_t code = 0, first = 0, index = 0;
  for (uint32_t len = 1; len <= 15; len++) {
    if (len > B.cnt) return D_TRUNCATED;
    code |= (uint32_t)(B.hold >> (len - 1)) & 1u;
    const uint32_t c = count[len];
    if (code - first < c) {
      B.drop(len);
      return sym[index + (code - first)];
    }
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  return D_NO_CODE;      // (not reached: a code with a hole is a single 1-bit code, and the lookup holds it)
}

RHI_HD void fixed_lengths(uint8_t* lens) {
  for (int i = 0; i < 144; i++) lens[i] = 8;
  for (int i = 144; i < 256; i++) lens[i] = 9;
  for (int i = 256; i < 280; i++) lens[i] = 7;
  for (int i = 280; i < 288; i++) lens[i] = 8;
  for (int i = 288; i < 320; i++) lens[i] = 5;
}

// the dynamic header, from behind the 3 block bits to both codes built
RHI_HD Status dynamic_header(Bits& B, Tables& T, bool writer) {
  if (!B.need(14)) return status(ST_TRUNCATED);
  const uint32_t nlen = B.peek(5) + 257, ndist = ((B.peek(10) >> 5) & 31) + 1, ncode = ((B.peek(14) >> 10) & 15) + 4;
  B.drop(14);
  if (nlen > 286 || ndist > 30) return status(ST_MALFORMED, R_TOO_MANY);
  RHI_SYNC();      // (loads of the last block's tables are done before the writer overwrites them)
  if (writer)
    for (int i = 0; i < 19; i++) T.clens[i] = 0;
  for (uint32_t i = 0; i < ncode; i++) {
    if (!B.need(3)) return status(ST_TRUNCATED);
    if (writer) T.clens[clen_order(i)] = (uint8_t)B.peek(3);
    B.drop(3);
  }
  RHI_SYNC();
  uint32_t r = build(T.clens, 19, T.ccount, T.csym, T.cfast, kClenBits, true, writer);
  if (r) return status(ST_MALFORMED, r, 0);
  RHI_SYNC();
  uint32_t have = 0, prev = 0;      // prev: lens[have - 1], kept in a register
  while (have < nlen + ndist) {
    int s = decode(B, T.ccount, T.csym, T.cfast, kClenBits);
    if (s == D_TRUNCATED) return status(ST_TRUNCATED);
    if (s == D_NO_CODE) s = 0;      // zlib: the 1-bit entry of a code-length code with no code at all reads as length 0
    if (s < 16) {
      if (writer) T.lens[have] = (uint8_t)s;
      have++;
      prev = (uint32_t)s;
      continue;
    }
    const uint32_t eb = s == 16 ? 2 : s == 17 ? 3 : 7, base = s == 18 ? 11 : 3;
    if (!B.need(eb)) return status(ST_TRUNCATED);
    if (s == 16 && have == 0) return status(ST_MALFORMED, R_REPEAT);
    const uint32_t v = s == 16 ? prev : 0, rep = base + B.peek(eb);
    B.drop(eb);
    if (have + rep > nlen + ndist) return status(ST_MALFORMED, R_REPEAT);      // (a run may cross from the literal/length lengths into the distance lengths)
    if (writer)
      for (uint32_t k = 0; k < rep; k++) T.lens[have + k] = (uint8_t)v;
    have += rep;
    prev = v;
  }
  RHI_SYNC();
  if (T.lens[256] == 0) return status(ST_MALFORMED, R_NO_EOB);
  r = build(T.lens, nlen, T.lcount, T.lsym, T.lfast, kLitBits, false, writer);
  if (r) return status(ST_MALFORMED, r, 1);
  r = build(T.lens + nlen, ndist, T.dcount, T.dsym, T.dfast, kDistBits, false, writer);
  if (r) return status(ST_MALFORMED, r, 2);
  if (writer) T.fixed_ready = 0;
  RHI_SYNC();
  return status(ST_OK);
}

// One raw-deflate stream.  ST_OK / ST_TRAILING: the stream is whole (TRAILING: detail = whole bytes behind the byte that holds
// its last bit -- zlib's unused_data); anything else: what stopped the walk.  max_out: ST_TOO_LARGE (detail = max_out) as soon
// as that many bytes are produced, whatever the stream still holds.  T: scratch (LDS on the device), T.fixed_ready = 0 at entry.
template <class Sink>
RHI_HD Status inflate_stream(const uint8_t* p, uint64_t len, Tables& T, Sink& out, uint64_t max_out, bool writer) {
  Bits B;
  B.init(p, len);
  for (;;) {
    if (!B.need(3)) return status(ST_TRUNCATED);
    const uint32_t last = B.peek(1), type = B.peek(3) >> 1;
    B.drop(3);
    if (type == 3) return status(ST_MALFORMED, R_BLOCK_TYPE);
    if (type == 0) {
      B.to_byte();
      if (!B.need(32)) return status(ST_TRUNCATED);
      const uint32_t v = B.peek(32);
      B.drop(32);
      if ((v & 0xFFFF) != ((v >> 16) ^ 0xFFFF)) return status(ST_MALFORMED, R_STORED_LEN);
      B.rewind();
      const uint64_t n = v & 0xFFFF, avail = len - B.pos, take = n < avail ? n : avail;
      if (out.produced() + take >= max_out) return status(ST_TOO_LARGE, R_NONE, max_out);
      if (!out.stored(p + B.pos, (uint32_t)take)) return status(ST_INTERNAL);
      B.pos += take;
      if (take < n) return status(ST_TRUNCATED);
    } else {
      if (type == 1) {
        RHI_SYNC();
        if (!T.fixed_ready) {
          RHI_SYNC();
          if (writer) fixed_lengths(T.lens);
          RHI_SYNC();
          build(T.lens, 288, T.lcount, T.lsym, T.lfast, kLitBits, false, writer);
          build(T.lens + 288, 32, T.dcount, T.dsym, T.dfast, kDistBits, false, writer);      // (symbols 30 and 31 have codes, and no meaning)
          if (writer) T.fixed_ready = 1;
          RHI_SYNC();
        }
      } else {
        const Status h = dynamic_header(B, T, writer);
        if (h.code != ST_OK) return h;
      }
      for (;;) {
        int s = decode(B, T.lcount, T.lsym, T.lfast, kLitBits);
        if (s == D_TRUNCATED) return status(ST_TRUNCATED);
        if (s == D_NO_CODE) return status(ST_MALFORMED, R_NO_CODE, 1);
        if (s < 256) {
          if (!out.lit((uint8_t)s)) return status(ST_INTERNAL);
        } else if (s == 256) {
          break;
        } else {
          if (s >= 286) return status(ST_MALFORMED, R_LITLEN_286);
          uint32_t eb = len_extra((uint32_t)s - 257);
          if (!B.need(eb)) return status(ST_TRUNCATED);
          const uint32_t length = len_base((uint32_t)s - 257) + B.peek(eb);      // (284 with 31 extra is 258 too)
          B.drop(eb);
          const int d = decode(B, T.dcount, T.dsym, T.dfast, kDistBits);
          if (d == D_TRUNCATED) return status(ST_TRUNCATED);
          if (d == D_NO_CODE) return status(ST_MALFORMED, R_NO_CODE, 2);
          if (d >= 30) return status(ST_MALFORMED, R_DIST_30);
          eb = dist_extra((uint32_t)d);
          if (!B.need(eb)) return status(ST_TRUNCATED);
          const uint32_t dist = dist_base((uint32_t)d) + B.peek(eb);
          B.drop(eb);
          if (dist > out.produced()) return status(ST_MALFORMED, R_TOO_FAR);
          if (!out.copy(length, dist)) return status(ST_INTERNAL);
        }
        if (out.produced() >= max_out) return status(ST_TOO_LARGE, R_NONE, max_out);
      }
    }
    if (last) break;
  }
  const uint64_t behind = len - B.bytes_used();
  return behind ? status(ST_TRAILING, R_NONE, behind) : status(ST_OK);
}

// the sink of a size walk: nothing is stored, a match needs no history to be counted
struct CountSink {
  uint64_t n = 0;
  RHI_HD bool lit(uint8_t) { n++; return true; }
  RHI_HD bool copy(uint32_t length, uint32_t) { n += length; return true; }
  RHI_HD bool stored(const uint8_t*, uint32_t k) { n += k; return true; }
  RHI_HD uint64_t produced() const { return n; }
};

}  // namespace rhi
