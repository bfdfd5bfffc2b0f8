// RFC 1951 raw deflate, the WRITING side, written once for the device (deflate.hip) and for the host (engine_deflate.cpp,
// tools/deflate_check.cpp): DESIGN.md 14.3, "Deflate blocks written on the device".  No HIP include is needed on the host side;
// not one of the headers the specialised kernels include, so the kernel-cache key does not see this file.
//
// SEGMENTS.  A payload (one container block) is cut into segments of kSegment bytes.  deflate_segment compresses ONE segment on
// its own -- no history from the segment before -- into whole deflate blocks.  Every segment but the last of a stream ends with
// an empty non-final stored block (3 zero bits, the padding, 00 00 FF FF: zlib's Z_SYNC_FLUSH marker), so segments end on a byte
// and are concatenated; the last one carries BFINAL.  An empty payload is one empty segment: one final fixed block, `03 00`.
//
// One code, two forms.  Every function takes a Ctx {lane, nl}: the host runs it with {0, 1}, the device with
// {threadIdx.x, 64} -- one wavefront, a workgroup of exactly that.  `for (i = X.lane; i < n; i += X.nl)` is a cooperative step:
// its turns are independent of each other, so the serial loop of the host and the 64 lanes of the device compute the same
// thing.  Everything else is wave-uniform: all lanes take the same control flow over the same values, only the writer (lane 0)
// stores into the tables of State (LDS on the device), and RHI_SYNC() stands between its stores and the other lanes' loads.
// The code build alone runs on the writer lane only (`if (writer)`): it is serial, its loads follow its own stores, and it
// holds no cooperative step; its results reach the other lanes through State behind a RHI_SYNC().
//
// LZ77 (lz_batch).  Defined in batches of 64 consecutive positions p .. p + 63.  (1) Each position hashes its next 3 bytes and
// looks up head[] AS IT STOOD BEFORE THE BATCH, verifies the candidate byte by byte, and notes (length, distance).  (2) All 64
// insert themselves; the table keeps the highest position per hash (atomicMax on the device, in position order on the host:
// the same table).  (3) A wave-uniform greedy pass walks the batch: a usable match is taken and its positions are skipped
// (it may run past the batch, never past the segment), otherwise one literal is emitted.  A match is 3 .. 258 bytes at
// distance 1 .. kSegment - 1 and never reaches in front of the segment's first byte: candidates are positions of this segment.
//
// HUFFMAN (flush_block).  The tokens wait in State::tok, 16-bit units: a literal (< 0x100), or a length unit (0x100 + length
// - 3) followed by a distance unit (0x8000 | distance - 1).  When the buffer is nearly full or the segment ends, the tokens
// become one deflate block in the cheapest of three forms by exact bit count -- stored, the fixed code, a dynamic code from the
// block's own histogram (length-limited to 15 bits; its code-length code to 7; lengths run-length coded with 16 / 17 / 18
// across the literal/length -- distance boundary; HCLEN trimmed in the permuted order).  Every code written is one zlib accepts:
// the literal/length code and the code-length code are complete (a code with one used symbol gets a second, unused one); the
// distance code is complete, or a single code of length 1 when exactly one distance symbol occurs, or one length of 0 when no
// match occurs.  `strategy` restricts the choice (1 stored, 2 fixed, 3 dynamic only) so that tests reach every writer.
//
// THE BOUND.  A segment of n bytes never takes more than n + 5 bytes in front of its marker: the exact cost of a block is known
// before its first bit is written, and a block that would pass 8 * (n + 5) bits in all makes the whole segment ONE stored
// block instead (n <= kSegment < 65,536: LEN fits), whatever `strategy` says -- the slot is the invariant, the strategy a wish.
// The marker adds at most 5 bytes (3 bits that may open a new byte, then 00 00 FF FF).  So
//     segment_bound(n, last) = n + 5 + (last ? 0 : 5)
//     deflate_bound(len)     = len + 10 * S - 5,   S = max(1, ceil(len / kSegment)) segments
// and deflate_bound(len) <= len + 16 * (len / 32768 + 1) because S <= len / 32768 + 1.
//
// TERMINATION AND BOUNDS.
//   - deflate_segment: the batch loop advances p by 64 per turn; the block loop runs at least one batch per turn (the token
//     buffer is empty behind a flush and a batch adds at most 128 units) or ends when p >= n.  At most n / 64 + 1 batches.
//   - lz_batch: three loops over 64; the verify loop advances `len` by 1 .. 8 per turn up to maxlen <= 258; the greedy loop
//     advances i by at least 1 per turn up to 64.
//   - build_lengths, rle_lengths, assign_codes: loops over at most 288 / 316 symbols and 15 lengths; the sort is a shell sort
//     over at most 288 keys; the length-limit loop lowers `total` by one per turn down to 2^maxbits.
//   - emit_units advances 64 units per turn; the stored copy advances at least 64 bytes per turn (reserve() makes room).
//   - Reads of input: position q is read only as in[q + k] with q + k < n (hash: q + 3 <= n; verify: k < maxlen <= n - q; the
//     candidate is in front of q); a stored copy reads [from, to) with to <= n.  Nothing is read outside [in, in + n).
//   - Stores: only Out::drain stores to the slot, and it refuses (Out::bad, nothing stored) what would pass `cap`; by the
//     accounting above that never happens for cap = segment_bound.  State arrays: tok[] is indexed below kTokUnits (a batch
//     starts only with 128 units free), stage[] below kStageWords + 8 (reserve() before every put), cl[] below 320.
#pragma once
#include <stdint.h>

#include "inflate_core.h"      // RHI_HD, RHI_SYNC, the base / extra-bit tables of RFC 1951 3.2.5, clen_order, fixed_lengths

namespace rhd {

constexpr uint32_t kSegment = 32768;          // every distance inside a segment is legal, a position fits 16 bits
constexpr uint32_t kBatch = 64;
constexpr uint32_t kHashBits = 12;
constexpr uint32_t kTokUnits = 4096;          // 16-bit units of the token buffer
constexpr uint32_t kStageWords = 512;         // the staging buffer of the bit writer, 32-bit words
constexpr uint32_t kStageBits = kStageWords * 32;
constexpr uint32_t kMinMatch = 3, kMaxMatch = 258;
constexpr uint32_t kFar3 = 4096;              // a match of 3 bytes further back than this costs more than its literals

enum : uint32_t { AUTO = 0, STORED = 1, FIXED = 2, DYNAMIC = 3 };

struct Ctx {
  uint32_t lane, nl;
};

RHI_HD uint64_t segments_of(uint64_t len) { return len ? (len + kSegment - 1) / kSegment : 1; }
RHI_HD uint64_t segment_bound(uint64_t n, bool last) { return n + 5 + (last ? 0 : 5); }
RHI_HD uint64_t deflate_bound(uint64_t len) { return len + 10 * segments_of(len) - 5; }

// ---- symbols of a length and of a distance: the inverse of rhi::len_base / dist_base (tools/deflate_check.cpp compares) -------
RHI_HD uint32_t len_sym(uint32_t length) {      // 3 .. 258 -> 0 .. 28
  if (length == 258) return 28;
  const uint32_t l = length - 3;
  if (l < 8) return l;
  const uint32_t k = 31u - (uint32_t)__builtin_clz(l);
  return 4 * k - 4 + ((l >> (k - 2)) & 3);
}
RHI_HD uint32_t dist_sym(uint32_t dist) {      // 1 .. 32768 -> 0 .. 29
  const uint32_t x = dist - 1;
  if (x < 4) return x;
  const uint32_t k = 31u - (uint32_t)__builtin_clz(x);
  return 2 * k + ((x >> (k - 1)) & 1);
}
RHI_HD uint32_t fixed_len(uint32_t s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }

struct State {
  uint32_t head[1u << kHashBits];      // position + 1 of the latest occurrence of a hash, 0 = none
  uint32_t stage[kStageWords + 8];     // the bits not yet drained; every word above the last bit is 0
  uint32_t key[288];                   // build_lengths
  uint32_t plan[8];                    // flush_block: what the writer lane decided (P_*)
  uint16_t tok[kTokUnits];
  uint16_t lfreq[288], dfreq[32], clfreq[20];
  uint16_t lcode[288], dcode[32], clcode[20];
  uint16_t sym[288];                   // build_lengths
  uint16_t cl[320];                    // the run-length coded lengths: symbol | extra << 5
  uint16_t mlen[kBatch], mdist[kBatch];
  uint8_t llen[288], dlen[32], cllen[20];
};
enum { P_FIXED = 0, P_DYN = 1, P_HLIT = 2, P_HDIST = 3, P_HCLEN = 4, P_NCL = 5 };

// ---- the bit writer: a staging buffer that drains into the segment's slot ------------------------------------------------------
// Bit k of the segment's output is bit (k & 31) of little-endian word k >> 5: byte k >> 3, LSB first, as RFC 1951 packs.
struct Out {
  uint8_t* o;           // the slot
  uint64_t cap;         // writable bytes at o
  uint64_t obytes;      // bytes drained (a multiple of 16 until the last drain)
  uint32_t sbits;       // bits in stage[]
  bool bad;             // a drain was refused: never by the accounting of the header comment

  RHI_HD uint64_t bits() const { return obytes * 8 + sbits; }

  RHI_HD void begin(State& S, const Ctx X, uint8_t* slot, uint64_t cap_) {
    o = slot; cap = cap_; obytes = 0; sbits = 0; bad = false;
    RHI_SYNC();
    for (uint32_t w = X.lane; w < kStageWords + 8; w += X.nl) S.stage[w] = 0;
    RHI_SYNC();
  }
  // Whole 16-byte pieces go to the slot (on the device in aligned 16-byte stores where the slot is aligned), the rest moves to
  // the front; final: every byte that holds a bit goes.
  RHI_HD void drain(State& S, const Ctx X, bool final) {
    RHI_SYNC();
    uint32_t nbytes = final ? (sbits + 7) >> 3 : (sbits >> 3) & ~15u;
    if (obytes + nbytes > cap) { bad = true; nbytes = 0; if (final) sbits = 0; }
    uint32_t nvec = nbytes >> 4;
#if defined(__HIP_DEVICE_COMPILE__)
    if (reinterpret_cast<uintptr_t>(o) & 15) nvec = 0;      // (obytes is a multiple of 16)
    for (uint32_t v = X.lane; v < nvec; v += X.nl)
      *reinterpret_cast<uint4*>(o + obytes + 16 * v) = *reinterpret_cast<const uint4*>(&S.stage[4 * v]);
#else
    for (uint32_t v = X.lane; v < nvec; v += X.nl) __builtin_memcpy(o + obytes + 16 * v, &S.stage[4 * v], 16);
#endif
    const uint8_t* s8 = reinterpret_cast<const uint8_t*>(S.stage);
    for (uint32_t i = (nvec << 4) + X.lane; i < nbytes; i += X.nl) o[obytes + i] = s8[i];
    const uint32_t from = nbytes >> 2, used = (sbits + 31) >> 5;      // (not final: nbytes is a multiple of 16, fewer than 128 bits stay)
    const uint32_t k0 = S.stage[from], k1 = S.stage[from + 1], k2 = S.stage[from + 2], k3 = S.stage[from + 3];
    RHI_SYNC();
    for (uint32_t w = X.lane; w < used; w += X.nl) S.stage[w] = final ? 0 : w == 0 ? k0 : w == 1 ? k1 : w == 2 ? k2 : w == 3 ? k3 : 0;
    RHI_SYNC();
    obytes += nbytes;
    sbits = final ? 0 : sbits - nbytes * 8;
  }
  RHI_HD void reserve(State& S, const Ctx X, uint32_t nbits) {      // nbits <= kStageBits - 128
    if (sbits + nbits > kStageBits) drain(S, X, false);
  }
  // n <= 32 bits by the writer lane (wave-uniform call; reserve() first)
  RHI_HD void put(State& S, const Ctx X, uint32_t v, uint32_t n) {
    if (X.lane == 0 && n) {
      const uint32_t w = sbits >> 5, sh = sbits & 31;
      S.stage[w] |= v << sh;
      if (sh + n > 32) S.stage[w + 1] |= v >> (32 - sh);
    }
    sbits += n;
  }
  RHI_HD void to_byte() { sbits = (sbits + 7) & ~7u; }
};

// ---- codes ---------------------------------------------------------------------------------------------------------------------
// Code lengths of at most `maxbits` bits for freq[0 .. n), into lens[] (0 = unused): a Huffman code by the in-place
// minimum-redundancy construction of Moffat and Katajainen over the sorted frequencies, then the lengths above maxbits are
// folded into it and the Kraft sum is repaired one unit per turn (a code of maxbits dropped, one shorter code split in two).
// pad: a code with fewer than two used symbols gets unused ones of frequency 1 (the lowest free symbols), so it is complete.
// Returns the number of codes.  0: no code; 1: lens[that] = 1 (incomplete; only with pad == false).  Serial: the writer lane.
RHI_HD uint32_t build_lengths(const uint16_t* freq, uint32_t n, uint32_t maxbits, bool pad, uint8_t* lens, uint32_t* key, uint16_t* sym) {
  uint32_t m = 0;
  for (uint32_t i = 0; i < n; i++) {
    lens[i] = 0;
    if (freq[i]) key[m++] = ((uint32_t)freq[i] << 9) | i;
  }
  if (pad)
    for (uint32_t s = 0; m < 2 && s < n; s++)
      if (!freq[s]) key[m++] = (1u << 9) | s;
  if (m == 0) return 0;
  if (m == 1) { lens[key[0] & 511] = 1; return 1; }
  for (uint32_t gap = 128; gap; gap = gap == 2 ? 1 : gap * 5 / 11) {      // shell sort, ascending by (frequency, symbol): keys are distinct
    for (uint32_t i = gap; i < m; i++) {
      const uint32_t v = key[i];
      uint32_t j = i;
      for (; j >= gap && key[j - gap] > v; j -= gap) key[j] = key[j - gap];
      key[j] = v;
    }
  }
  for (uint32_t i = 0; i < m; i++) { sym[i] = (uint16_t)(key[i] & 511); key[i] >>= 9; }
  // phase 1: internal nodes' weights, then parents; phase 2: depths of internal nodes; phase 3: depths of leaves
  key[0] += key[1];
  uint32_t root = 0, leaf = 2;
  for (uint32_t next = 1; next + 1 < m; next++) {
    if (leaf >= m || key[root] < key[leaf]) { key[next] = key[root]; key[root++] = next; }
    else key[next] = key[leaf++];
    if (leaf >= m || (root < next && key[root] < key[leaf])) { key[next] += key[root]; key[root++] = next; }
    else key[next] += key[leaf++];
  }
  key[m - 2] = 0;
  for (int next = (int)m - 3; next >= 0; next--) key[next] = key[key[next]] + 1;
  {
    int avbl = 1, used = 0, rt = (int)m - 2, nx = (int)m - 1;
    uint32_t dpth = 0;
    while (avbl > 0) {
      while (rt >= 0 && key[rt] == dpth) { used++; rt--; }
      while (avbl > used) { key[nx--] = dpth; avbl--; }
      avbl = 2 * used; dpth++; used = 0;
    }
  }
  uint32_t cnt[16];
  for (uint32_t l = 0; l < 16; l++) cnt[l] = 0;
  for (uint32_t i = 0; i < m; i++) cnt[key[i] > maxbits ? maxbits : key[i]]++;
  uint32_t total = 0;
  for (uint32_t l = maxbits; l > 0; l--) total += cnt[l] << (maxbits - l);
  while (total != (1u << maxbits)) {
    cnt[maxbits]--;
    for (uint32_t l = maxbits - 1; l > 0; l--)
      if (cnt[l]) { cnt[l]--; cnt[l + 1] += 2; break; }
    total--;
  }
  uint32_t j = m;      // sym[] ascends by frequency: the rarest take the longest codes
  for (uint32_t l = 1; l <= maxbits; l++)
    for (uint32_t c = cnt[l]; c > 0; c--) lens[sym[--j]] = (uint8_t)l;
  return m;
}

// canonical codes of RFC 1951 3.2.2, stored bit-reversed: ready to be put LSB first.  Serial: the writer lane.
RHI_HD void assign_codes(const uint8_t* lens, uint32_t n, uint16_t* code) {
  uint32_t cnt[16], next[16];
  for (uint32_t l = 0; l < 16; l++) cnt[l] = 0;
  for (uint32_t i = 0; i < n; i++) cnt[lens[i] & 15]++;
  cnt[0] = 0;
  uint32_t c = 0;
  next[0] = 0;
  for (uint32_t l = 1; l < 16; l++) { c = (c + cnt[l - 1]) << 1; next[l] = c; }
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t l = lens[i] & 15;
    uint32_t v = l ? next[l]++ : 0, r = 0;
    for (uint32_t b = 0; b < l; b++) r |= ((v >> b) & 1u) << (l - 1 - b);
    code[i] = (uint16_t)r;
  }
}

// The lengths llen[0 .. hlit) then dlen[0 .. hdist) run-length coded into S.cl / S.clfreq; returns the number of entries.
RHI_HD uint32_t rle_lengths(State& S, uint32_t hlit, uint32_t hdist) {
  for (uint32_t i = 0; i < 20; i++) S.clfreq[i] = 0;
  const uint32_t n = hlit + hdist;
  uint32_t k = 0, i = 0;
  while (i < n) {
    const uint32_t v = i < hlit ? S.llen[i] : S.dlen[i - hlit];
    uint32_t run = 1;
    while (i + run < n && (i + run < hlit ? S.llen[i + run] : S.dlen[i + run - hlit]) == v) run++;
    i += run;
    if (v == 0) {
      while (run >= 11) { const uint32_t r = run < 138 ? run : 138; S.cl[k++] = (uint16_t)(18 | ((r - 11) << 5)); S.clfreq[18]++; run -= r; }
      if (run >= 3) { S.cl[k++] = (uint16_t)(17 | ((run - 3) << 5)); S.clfreq[17]++; run = 0; }
    } else {
      S.cl[k++] = (uint16_t)v; S.clfreq[v]++; run--;
      while (run >= 3) { const uint32_t r = run < 6 ? run : 6; S.cl[k++] = (uint16_t)(16 | ((r - 3) << 5)); S.clfreq[16]++; run -= r; }
    }
    for (; run; run--) { S.cl[k++] = (uint16_t)v; S.clfreq[v]++; }
  }
  return k;
}

// The dynamic code of the block's histogram and its header, planned: lengths, run-length coding, the code-length code, HLIT /
// HDIST / HCLEN and the block's exact size in bits behind the 3 block bits.  Serial: the writer lane.  `extra`: the extra
// bits of the block's lengths and distances.
RHI_HD void plan_dynamic(State& S, uint32_t extra) {
  build_lengths(S.lfreq, 286, 15, true, S.llen, S.key, S.sym);
  build_lengths(S.dfreq, 30, 15, false, S.dlen, S.key, S.sym);
  uint32_t hlit = 286, hdist = 30;
  while (hlit > 257 && S.llen[hlit - 1] == 0) hlit--;
  while (hdist > 1 && S.dlen[hdist - 1] == 0) hdist--;
  const uint32_t ncl = rle_lengths(S, hlit, hdist);
  build_lengths(S.clfreq, 19, 7, true, S.cllen, S.key, S.sym);
  assign_codes(S.cllen, 19, S.clcode);
  uint32_t hclen = 19;
  while (hclen > 4 && S.cllen[rhi::clen_order(hclen - 1)] == 0) hclen--;
  uint32_t bits = 14 + 3 * hclen + extra;
  for (uint32_t k = 0; k < ncl; k++) {
    const uint32_t s = S.cl[k] & 31;
    bits += S.cllen[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0);
  }
  for (uint32_t s = 0; s < 286; s++) bits += (uint32_t)S.lfreq[s] * S.llen[s];
  for (uint32_t s = 0; s < 30; s++) bits += (uint32_t)S.dfreq[s] * S.dlen[s];
  S.plan[P_DYN] = bits; S.plan[P_HLIT] = hlit; S.plan[P_HDIST] = hdist; S.plan[P_HCLEN] = hclen; S.plan[P_NCL] = ncl;
}

// the bits of one token unit under the codes in State
RHI_HD void unit_bits(const State& S, uint32_t u, uint32_t& v, uint32_t& nb) {
  if (u < 0x100) { v = S.lcode[u]; nb = S.llen[u]; return; }
  if (u < 0x8000) {
    const uint32_t length = u - 0x100 + 3, s = len_sym(length), l = S.llen[257 + s];
    v = S.lcode[257 + s] | ((length - rhi::len_base(s)) << l);
    nb = l + rhi::len_extra(s);
    return;
  }
  const uint32_t dist = (u & 0x7FFF) + 1, s = dist_sym(dist), l = S.dlen[s];
  v = S.dcode[s] | ((dist - rhi::dist_base(s)) << l);
  nb = l + rhi::dist_extra(s);
}

// The units tok[0 .. nunits) as bits, 64 per step: each unit's bits (at most 28) land at the prefix sum of the bit counts in
// front of it.  The host form is the loop; the device form gives a lane a unit, scans the counts across the wavefront and ORs
// into the staging words (two neighbours share a word: atomicOr).  Bits are the same wherever they are ORed from.
RHI_HD void emit_units(State& S, const Ctx X, Out& out, uint32_t nunits) {
  for (uint32_t base = 0; base < nunits; base += kBatch) {
    out.reserve(S, X, kBatch * 28);
    RHI_SYNC();
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = base + X.lane;
    uint32_t v = 0, nb = 0;
    if (i < nunits) unit_bits(S, S.tok[i], v, nb);
    uint32_t inc = nb;
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const uint32_t t = __shfl_up(inc, d, 64);
      if (X.lane >= d) inc += t;
    }
    const uint32_t total = __shfl(inc, 63, 64), at = out.sbits + inc - nb;
    if (nb) {
      const uint32_t w = at >> 5, sh = at & 31;
      atomicOr(&S.stage[w], v << sh);
      if (sh + nb > 32) atomicOr(&S.stage[w + 1], v >> (32 - sh));
    }
    out.sbits += total;
#else
    const uint32_t to = base + kBatch < nunits ? base + kBatch : nunits;
    for (uint32_t i = base; i < to; i++) {
      uint32_t v, nb;
      unit_bits(S, S.tok[i], v, nb);
      out.put(S, X, v, nb);
    }
#endif
    RHI_SYNC();
  }
}

// in[from .. to) as one stored block (to - from <= 65,535)
RHI_HD void put_stored(State& S, const Ctx X, Out& out, const uint8_t* in, uint32_t from, uint32_t to, bool final) {
  const uint32_t n = to - from;
  out.reserve(S, X, 48);
  RHI_SYNC();
  out.put(S, X, final ? 1 : 0, 3);
  out.to_byte();
  out.put(S, X, n | ((~n & 0xFFFFu) << 16), 32);
  RHI_SYNC();
  uint8_t* s8 = reinterpret_cast<uint8_t*>(S.stage);
  for (uint32_t done = 0; done < n;) {
    out.reserve(S, X, 8 * 64);
    const uint32_t room = (kStageBits - out.sbits) >> 3, c = n - done < room ? n - done : room, at = out.sbits >> 3;
    for (uint32_t i = X.lane; i < c; i += X.nl) s8[at + i] = in[from + done + i];
    out.sbits += 8 * c;
    done += c;
    RHI_SYNC();
  }
}

// ---- LZ77 ----------------------------------------------------------------------------------------------------------------------
struct Lz {
  uint32_t cursor;      // the first position no token covers yet
  uint32_t ntok;        // units in tok[]
  uint32_t extra;       // extra bits of the block's lengths and distances
  uint32_t fixed;       // the block's tokens under the fixed code, in bits
};

RHI_HD uint32_t hash3(const uint8_t* p) {
  const uint32_t v = p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
  return (v * 0x9E3779B1u) >> (32 - kHashBits);
}

RHI_HD void lz_batch(State& S, const Ctx X, const uint8_t* in, uint32_t n, uint32_t p, Lz& z) {
  // (1) look up and verify: the table as it stood before the batch
  for (uint32_t i = X.lane; i < kBatch; i += X.nl) {
    const uint32_t q = p + i;
    uint32_t len = 0, dist = 0;
    if (q + kMinMatch <= n) {
      const uint32_t c = S.head[hash3(in + q)];
      if (c) {
        const uint32_t cand = c - 1, maxlen = n - q < kMaxMatch ? n - q : kMaxMatch;      // cand < p <= q
        while (len + 8 <= maxlen) {
          uint64_t a, b;
          __builtin_memcpy(&a, in + cand + len, 8);
          __builtin_memcpy(&b, in + q + len, 8);
          if (a != b) { len += (uint32_t)__builtin_ctzll(a ^ b) >> 3; break; }
          len += 8;
        }
        if (len + 8 > maxlen)      // (the tail, or nothing: a mismatch above left len + 8 <= maxlen)
          while (len < maxlen && in[cand + len] == in[q + len]) len++;
        dist = q - cand;
        if (len < kMinMatch || (len == kMinMatch && dist > kFar3)) len = 0;
      }
    }
    S.mlen[i] = (uint16_t)len;
    S.mdist[i] = (uint16_t)dist;
  }
  RHI_SYNC();
  // (2) insert, in position order: the highest position of a hash stays
  for (uint32_t i = X.lane; i < kBatch; i += X.nl) {
    const uint32_t q = p + i;
    if (q + kMinMatch <= n) {
      uint32_t* h = &S.head[hash3(in + q)];
#if defined(__HIP_DEVICE_COMPILE__)
      atomicMax(h, q + 1);
#else
      if (*h < q + 1) *h = q + 1;
#endif
    }
  }
  RHI_SYNC();
  // (3) the greedy pass: wave-uniform, the writer lane stores
  const bool writer = X.lane == 0;
  uint32_t i = z.cursor > p ? z.cursor - p : 0;
  while (i < kBatch && p + i < n) {
    const uint32_t len = S.mlen[i];
    if (len) {
      const uint32_t dist = S.mdist[i], ls = len_sym(len), ds = dist_sym(dist);
      if (writer) {
        S.tok[z.ntok] = (uint16_t)(0x100 + len - 3);
        S.tok[z.ntok + 1] = (uint16_t)(0x8000 | (dist - 1));
        S.lfreq[257 + ls]++;
        S.dfreq[ds]++;
      }
      z.ntok += 2;
      z.extra += rhi::len_extra(ls) + rhi::dist_extra(ds);
      z.fixed += fixed_len(257 + ls) + 5;
      i += len;
    } else {
      const uint32_t b = in[p + i];
      if (writer) { S.tok[z.ntok] = (uint16_t)b; S.lfreq[b]++; }
      z.ntok += 1;
      z.fixed += fixed_len(b);
      i++;
    }
  }
  z.cursor = p + i;
  RHI_SYNC();
}

RHI_HD void clear_block(State& S, const Ctx X, Lz& z) {
  RHI_SYNC();
  for (uint32_t s = X.lane; s < 288; s += X.nl) S.lfreq[s] = 0;
  for (uint32_t s = X.lane; s < 32; s += X.nl) S.dfreq[s] = 0;
  RHI_SYNC();
  z.ntok = 0; z.extra = 0; z.fixed = 0;
}

// The tokens of in[from .. to) as one deflate block in the cheapest form `strategy` admits.  false: the block would take the
// segment past `limit` bits in all; nothing was written.
RHI_HD bool flush_block(State& S, const Ctx X, Out& out, const uint8_t* in, uint32_t from, uint32_t to, const Lz& z, bool final, uint32_t strategy,
                        uint64_t limit) {
  const bool writer = X.lane == 0;
  const bool want_dyn = strategy == AUTO || strategy == DYNAMIC;
  RHI_SYNC();
  if (writer) {
    S.lfreq[256]++;      // end of block
    S.plan[P_FIXED] = z.fixed + z.extra + 7;
    if (want_dyn) plan_dynamic(S, z.extra);
  }
  RHI_SYNC();
  const uint64_t at = out.bits();
  const uint64_t c_stored = ((at + 3 + 7) & ~7ull) - at + 32 + 8ull * (to - from);
  const uint64_t c_fixed = 3 + (uint64_t)S.plan[P_FIXED], c_dyn = want_dyn ? 3 + (uint64_t)S.plan[P_DYN] : ~0ull;
  uint32_t form;
  uint64_t cost;
  if (strategy == FIXED) { form = FIXED; cost = c_fixed; }
  else if (strategy == DYNAMIC) { form = DYNAMIC; cost = c_dyn; }
  else {
    form = FIXED; cost = c_fixed;
    if (c_dyn < cost) { form = DYNAMIC; cost = c_dyn; }
    if (c_stored < cost) { form = STORED; cost = c_stored; }
  }
  if (at + cost > limit) return false;
  if (form == STORED) {
    put_stored(S, X, out, in, from, to, final);
    return true;
  }
  if (writer) {
    if (form == FIXED) {
      for (uint32_t s = 0; s < 288; s++) S.llen[s] = (uint8_t)fixed_len(s);
      for (uint32_t s = 0; s < 32; s++) S.dlen[s] = 5;
    }
    assign_codes(S.llen, form == FIXED ? 288 : 286, S.lcode);      // (a dynamic code has lengths for 286 / 30 symbols only)
    assign_codes(S.dlen, form == FIXED ? 32 : 30, S.dcode);
  }
  out.reserve(S, X, 8192);      // the header: 17 + 57 + 316 * 14 bits at most
  RHI_SYNC();
  out.put(S, X, (final ? 1u : 0u) | (form == FIXED ? 2u : 4u), 3);
  if (form == DYNAMIC) {
    const uint32_t hlit = S.plan[P_HLIT], hdist = S.plan[P_HDIST], hclen = S.plan[P_HCLEN], ncl = S.plan[P_NCL];
    out.put(S, X, (hlit - 257) | ((hdist - 1) << 5) | ((hclen - 4) << 10), 14);
    for (uint32_t k = 0; k < hclen; k++) out.put(S, X, S.cllen[rhi::clen_order(k)], 3);
    for (uint32_t k = 0; k < ncl; k++) {
      const uint32_t e = S.cl[k], s = e & 31, l = S.cllen[s];
      out.put(S, X, S.clcode[s] | ((e >> 5) << l), l + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0));
    }
  }
  RHI_SYNC();
  emit_units(S, X, out, z.ntok);
  out.reserve(S, X, 16);
  RHI_SYNC();
  out.put(S, X, S.lcode[256], S.llen[256]);
  RHI_SYNC();
  return true;
}

// One segment: in[0 .. n), n <= kSegment, into `slot` of segment_bound(n, last) bytes (on the device: any slot at least that
// large).  Returns the bytes written.  S: scratch (LDS on the device), nothing in it is kept between segments.
RHI_HD uint64_t deflate_segment(State& S, const Ctx X, const uint8_t* in, uint32_t n, bool last, uint32_t strategy, uint8_t* slot, uint64_t cap, bool* bad) {
  const uint64_t limit = 8ull * (n + 5);
  Out out;
  out.begin(S, X, slot, cap);
  bool whole = strategy != STORED;
  if (whole) {
    for (uint32_t h = X.lane; h < (1u << kHashBits); h += X.nl) S.head[h] = 0;
    Lz z;
    z.cursor = 0;
    clear_block(S, X, z);
    uint32_t p = 0, from = 0;
    for (;;) {
      while (p < n && z.ntok + 2 * kBatch <= kTokUnits) {
        lz_batch(S, X, in, n, p, z);
        p += kBatch;
      }
      const bool final_block = p >= n;      // (then the cursor stands at n)
      if (!flush_block(S, X, out, in, from, z.cursor, z, final_block && last, strategy, limit)) { whole = false; break; }
      if (final_block) break;
      from = z.cursor;
      clear_block(S, X, z);
    }
  }
  if (!whole) {      // the strategy is STORED, or the segment does not fit its slot in the form wanted: one stored block
    out.begin(S, X, slot, cap);
    put_stored(S, X, out, in, 0, n, last);
  }
  if (!last) {      // the marker: an empty stored block, not final
    out.reserve(S, X, 48);
    RHI_SYNC();
    out.put(S, X, 0, 3);
    out.to_byte();
    out.put(S, X, 0xFFFF0000u, 32);
    RHI_SYNC();
  }
  out.drain(S, X, true);
  if (out.bad) *bad = true;
  return out.obytes;
}

// One stream on the calling thread: len bytes at `in` into deflate_bound(len) bytes at `out`.  Returns its size, or ~0 if a
// store was refused (never: the accounting of the header comment).
inline uint64_t deflate_stream_host(State& S, const uint8_t* in, uint64_t len, uint32_t strategy, uint8_t* out) {
  const Ctx X = {0, 1};
  const uint64_t ns = segments_of(len);
  uint64_t pos = 0;
  bool bad = false;
  for (uint64_t k = 0; k < ns; k++) {
    const uint64_t at = k * kSegment, n = len - at < kSegment ? len - at : kSegment;
    const bool last = k + 1 == ns;
    pos += deflate_segment(S, X, in + at, (uint32_t)n, last, strategy, out + pos, segment_bound(n, last), &bad);
  }
  return bad ? ~0ull : pos;
}

}  // namespace rhd
