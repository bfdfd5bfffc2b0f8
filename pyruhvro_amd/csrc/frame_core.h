// Framed messages (rh_frame_*): the two framings, how a header is read and classified, the verdict codes, and the
// arithmetic of the stable multi-way partition.  Free of HIP and shared by the host (engine_frame.cpp, tools/frame_check.cpp) and
// the device (frame.hip), like filter_core.h: the byte order of an id and the place a message lands are stated here once and
// nowhere else.  Not one of the headers the specialised kernels include: the kernel-cache key does not see this file.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RFR_HD __host__ __device__
#else
#define RFR_HD
#endif

namespace rh {

constexpr uint32_t kMaxFrameIds = 32;       // writer schemas per call
constexpr uint32_t kFrameTile = 256;        // messages per tile: one workgroup of the classify and offsets kernels
constexpr uint32_t kFrameMaxHeader = 10;

enum FrameKind : uint32_t {
  FRAME_CONFLUENT = 0,       // 00 | id: 4 bytes, big-endian | datum
  FRAME_SINGLE_OBJECT = 1,   // C3 01 | CRC-64-AVRO fingerprint of the writer schema: 8 bytes, little-endian | datum
  FRAME_KINDS = 2,
};

struct FrameDesc {
  uint32_t header;           // bytes in front of the datum
  uint32_t marker_len;       // ... of which the marker
  uint32_t id_len;           // ... and the id behind it
  uint32_t big_endian;       // the id's byte order
  uint32_t marker0, marker1; // the marker's bytes (marker1 unused when marker_len is 1)
};

RFR_HD inline FrameDesc frame_desc(uint32_t kind) {
  FrameDesc d;
  if (kind == FRAME_SINGLE_OBJECT) {
    d.header = 10; d.marker_len = 2; d.id_len = 8; d.big_endian = 0; d.marker0 = 0xC3; d.marker1 = 0x01;
  } else {
    d.header = 5; d.marker_len = 1; d.id_len = 4; d.big_endian = 1; d.marker0 = 0x00; d.marker1 = 0x00;
  }
  return d;
}

// verdict of one message, one byte: its class (the position of its id in the call's ascending id list), or one of these
constexpr uint8_t kFrameUnknown = 0xFD;     // well framed, the id is not in the list
constexpr uint8_t kFrameShort = 0xFE;       // shorter than the header
constexpr uint8_t kFrameBadMarker = 0xFF;   // does not start with the marker
constexpr uint64_t kFrameNoFailure = ~0ull; // the lowest failing index when nothing failed

// `p`: the first byte of a message of at least d.header bytes.  Reads bytes [0, d.header) singly: no alignment is assumed.
RFR_HD inline bool frame_marker_ok(const uint8_t* p, const FrameDesc& d) {
  return p[0] == d.marker0 && (d.marker_len < 2 || p[1] == d.marker1);
}
RFR_HD inline uint64_t frame_id(const uint8_t* p, const FrameDesc& d) {
  uint64_t id = 0;
  for (uint32_t i = 0; i < d.id_len; i++) {
    const uint64_t b = p[d.marker_len + i];
    id = d.big_endian ? (id << 8) | b : id | (b << (8u * i));
  }
  return id;
}
// position of `id` in ids[0 .. m), ascending and distinct, m <= kMaxFrameIds; kFrameUnknown when it is not there.  Six turns
// whatever the id is: on the device the trip count is uniform.
RFR_HD inline uint8_t frame_class(const uint64_t* ids, uint32_t m, uint64_t id) {
  uint32_t lo = 0, hi = m;      // the first position whose id is >= `id` lies in [lo, hi]
  for (uint32_t turn = 0; turn < 6; turn++) {
    if (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (ids[mid] < id) lo = mid + 1;
      else hi = mid;
    }
  }
  return (lo < m && ids[lo] == id) ? (uint8_t)lo : kFrameUnknown;
}
// the verdict of the message data[b, e)
RFR_HD inline uint8_t frame_verdict(const uint8_t* data, uint64_t b, uint64_t e, const FrameDesc& d, const uint64_t* ids, uint32_t m) {
  if (e - b < d.header) return kFrameShort;
  if (!frame_marker_ok(data + b, d)) return kFrameBadMarker;
  return frame_class(ids, m, frame_id(data + b, d));
}

// ---------------------------------------------------------------------------
// The stable partition.  The messages go into m + 1 bins: bin c < m holds class c, bin m the messages with an unknown id (their
// indices are reported, they have no payload).  A message of a failing verdict is in no bin: such a call ends before it partitions.
// Tiles of kFrameTile messages; tables are bin-major, table[bin * ntiles + tile].
//   tile_cnt / tile_bytes   messages and payload bytes (length minus header) of the bin in the tile          (classify)
//   pre_cnt / pre_bytes     their exclusive prefixes over the tiles of one bin; the bin's totals beside them  (scan)
// Message i of bin c, the r-th of its bin in its tile with q payload bytes of the bin in front of it in the tile, lands at
//   rank = pre_cnt[c][tile] + r      in the bin's index list and offsets list
//   byte = pre_bytes[c][tile] + q    in the bin's payload region
// ---------------------------------------------------------------------------
RFR_HD inline uint32_t frame_bin(uint8_t verdict, uint32_t m) { return verdict < m ? (uint32_t)verdict : verdict == kFrameUnknown ? m : m + 1; }
RFR_HD inline uint64_t frame_tiles(uint64_t n) { return (n + kFrameTile - 1) / kFrameTile; }
RFR_HD inline uint64_t frame_table_at(uint64_t ntiles, uint32_t bin, uint64_t tile) { return (uint64_t)bin * ntiles + tile; }
RFR_HD inline uint64_t frame_payload_len(uint64_t b, uint64_t e, uint32_t bin, uint32_t m, const FrameDesc& d) {
  return bin < m ? (e - b) - d.header : 0;
}
RFR_HD inline uint64_t frame_rank(uint64_t pre_cnt, uint64_t rank_in_tile) { return pre_cnt + rank_in_tile; }
RFR_HD inline uint64_t frame_byte(uint64_t pre_bytes, uint64_t bytes_in_tile) { return pre_bytes + bytes_in_tile; }
// every bin's region starts 16-byte aligned in a lease of its own and is followed by this many zero bytes
constexpr uint64_t kFrameSlack = 64;

// ---------------------------------------------------------------------------
// The gather.  One wavefront per 64 messages, in kFrameRounds rounds: in round k the kFrameGroup lanes of group g copy the payload
// of message kFrameGroups * k + g of the wavefront.  A payload of `len` bytes whose destination address is `dst`: `head` single
// bytes up to the first 16-byte boundary of the DESTINATION, `nvec` 16-byte vectors (aligned stores, unaligned loads), `tail`
// single bytes; lane `sub` of the group takes byte `sub` of head and tail and the vectors sub, sub + kFrameGroup, ...
// ---------------------------------------------------------------------------
constexpr uint32_t kFrameGroup = 16;
constexpr uint32_t kFrameGroups = 64 / kFrameGroup;
constexpr uint32_t kFrameRounds = 64 / kFrameGroups;
struct FrameCopy {
  uint64_t head, nvec, tail;
};
RFR_HD inline FrameCopy frame_copy_plan(uint64_t dst, uint64_t len) {
  FrameCopy c;
  const uint64_t mis = (16u - (uint32_t)(dst & 15u)) & 15u;
  c.head = mis < len ? mis : len;
  c.nvec = (len - c.head) >> 4;
  c.tail = len - c.head - (c.nvec << 4);      // fewer than 16
  return c;
}

}  // namespace rh
