// Framed messages, the write side (rh_frame_join): the header a message gets, where a source row lands, the
// permutation's verdicts and the copy plan of one message.  Free of HIP and shared by the host (engine_frame_join.cpp,
// tools/frame_join_check.cpp) and the device (frame_join.hip), like frame_core.h, whose FrameDesc and frame_copy_plan it uses: the
// byte order of an id is stated there for the reader and here for the writer, and the check reads the one with the other.  Not one
// of the headers the specialised kernels include: the kernel-cache key does not see this file.
#pragma once
#include <stdint.h>

#include "frame_core.h"

namespace rh {

constexpr uint32_t kJoinTile = 256;           // messages per tile: one workgroup of every join kernel
constexpr uint64_t kJoinNone = ~0ull;         // a verdict word when nothing offended

// One source: the datums of one chunk of an encode result, `rows` of them, in the order of their rows.  The table lies in device
// memory, ordered as the caller gave the sources; row_end is the running row count through this source, so source row r (counted
// over all sources) belongs to the first source whose row_end is above r.
struct JoinSource {
  const int32_t* off;        // rows + 1 offsets into data (a BinaryArray's)
  const uint8_t* data;
  uint64_t row_end;
  uint64_t id;               // the wire id its messages carry
  uint64_t data_bytes;       // what the offsets may address
};

// byte i < d.header of the header in front of a datum of writer schema `id`
RFR_HD inline uint8_t join_header_byte(const FrameDesc& d, uint64_t id, uint32_t i) {
  if (i < d.marker_len) return (uint8_t)(i == 0 ? d.marker0 : d.marker1);
  const uint32_t b = i - d.marker_len;                                   // byte b of the id as the wire has it
  const uint32_t shift = 8u * (d.big_endian ? d.id_len - 1u - b : b);
  return (uint8_t)(id >> shift);
}

// the turns join_source_of needs for a table of nsrc entries (the same for every lane)
RFR_HD inline uint32_t join_search_turns(uint32_t nsrc) {
  uint32_t t = 0;
  while ((1ull << t) < (uint64_t)nsrc + 1) t++;
  return t;
}
// the first source whose row_end is above r; r is below the last row_end.  Sources of no rows are never found.
RFR_HD inline uint32_t join_source_of(const JoinSource* src, uint32_t nsrc, uint64_t r, uint32_t turns) {
  uint32_t lo = 0, hi = nsrc - 1;      // the answer lies in [lo, hi]
  for (uint32_t t = 0; t < turns; t++) {
    if (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (src[mid].row_end > r) hi = mid;
      else lo = mid + 1;
    }
  }
  return lo;
}
RFR_HD inline uint64_t join_row_in_source(const JoinSource* src, uint32_t s, uint64_t r) { return r - (s ? src[s - 1].row_end : 0); }

// ---------------------------------------------------------------------------
// The chunks of the result: k of them, the first k - 1 of sz messages, the last takes the remainder (what rh_encode gives n rows).
// ---------------------------------------------------------------------------
RFR_HD inline uint64_t join_tiles(uint64_t n) { return (n + kJoinTile - 1) / kJoinTile; }
RFR_HD inline uint32_t join_chunk_of(uint64_t p, uint64_t sz, uint32_t k) {
  const uint64_t c = p / sz;
  return c < k ? (uint32_t)c : k - 1;
}
RFR_HD inline uint64_t join_chunk_start(uint32_t c, uint64_t sz) { return (uint64_t)c * sz; }
// message p opens a chunk: its absolute byte offset is that chunk's base
RFR_HD inline bool join_opens_chunk(uint64_t p, uint64_t sz, uint32_t k) { return p % sz == 0 && p / sz < k; }
// message p closes its chunk: the entry behind its own offset is the chunk's total
RFR_HD inline bool join_closes_chunk(uint64_t p, uint64_t n, uint64_t sz, uint32_t k) { return p + 1 == n || join_opens_chunk(p + 1, sz, k); }

// ---------------------------------------------------------------------------
// The permutation.  Every row claims its position in a bitmap of n bits (one atomic OR on the device); a row that finds the bit
// set names a position a second time.  A position below n that nobody claimed is a hole.  Out-of-range indices are judged first
// (the lowest source row decides), then the lowest position that is not named exactly once.
// ---------------------------------------------------------------------------
RFR_HD inline uint64_t join_claim_words(uint64_t n) { return (n + 31) >> 5; }
RFR_HD inline uint64_t join_claim_word(uint64_t p) { return p >> 5; }
RFR_HD inline uint32_t join_claim_bit(uint64_t p) { return 1u << (uint32_t)(p & 31u); }
RFR_HD inline bool join_in_range(int64_t v, uint64_t n) { return v >= 0 && (uint64_t)v < n; }
// the lowest position whose bit is clear (the host reads the bitmap back only when a call fails)
inline uint64_t join_lowest_hole(const uint32_t* claim, uint64_t n) {
  for (uint64_t w = 0; w < join_claim_words(n); w++) {
    if (claim[w] == 0xFFFFFFFFu) continue;
    for (uint32_t b = 0; b < 32; b++) {
      const uint64_t p = (w << 5) + b;
      if (p >= n) return kJoinNone;
      if (!(claim[w] & (1u << b))) return p;
    }
  }
  return kJoinNone;
}
enum JoinVerdict : uint32_t { JOIN_OK = 0, JOIN_TWICE = 1, JOIN_NEVER = 2 };
// `twice`: the lowest position named more than once; `never`: the lowest hole (kJoinNone: none).  The lower of the two decides.
RFR_HD inline JoinVerdict join_perm_verdict(uint64_t twice, uint64_t never, uint64_t* at) {
  if (twice == kJoinNone && never == kJoinNone) return JOIN_OK;
  if (never < twice) { *at = never; return JOIN_NEVER; }
  *at = twice;
  return JOIN_TWICE;
}

// ---------------------------------------------------------------------------
// The gather.  One 16-lane group per message (frame_core.h kFrameGroup), four per wavefront.  A message of header h and a datum
// of `len` bytes whose destination ADDRESS is dst: lane sub < h writes header byte sub at dst + sub; the datum goes to dst + h by
// frame_copy_plan(dst + h, len): single bytes up to the first 16-byte boundary of the destination, 16-byte vectors (aligned
// stores, unaligned loads that stay inside the datum), single bytes behind them.
// ---------------------------------------------------------------------------
RFR_HD inline FrameCopy join_copy_plan(uint64_t dst, const FrameDesc& d, uint64_t len) { return frame_copy_plan(dst + d.header, len); }

}  // namespace rh
