// Framed messages (rh_frame_*): parameters of the kernels of frame.hip, shared by host and device code.  Not one of the headers
// the specialised kernels include: the kernel-cache key does not see this file.
#pragma once
#include <stdint.h>
#include "frame_core.h"

namespace rh {

constexpr uint32_t kFrameBins = kMaxFrameIds + 1;      // the classes and, last, the messages with an unknown id

// classify -> scan -> (the host reads the totals and leases every class its region) -> offsets -> gather
struct FrameParams {
  const uint8_t* data;       // packed messages (16-byte aligned)
  const uint64_t* offsets;   // n + 1 message offsets into data
  uint64_t data_len;
  uint64_t n;
  uint64_t ntiles;           // frame_tiles(n)
  uint32_t kind;             // FrameKind
  uint32_t m;                // ids in the call, 1 .. kMaxFrameIds
  uint32_t skip_unknown;     // an unknown id is no failure: the message goes to bin m
  uint32_t pad;
  uint64_t ids[kMaxFrameIds];              // ascending, distinct
  uint8_t* cls;                            // [n] verdicts
  unsigned long long* first_bad;           // the lowest failing index (kFrameNoFailure at launch)
  uint64_t* tile_cnt;                      // [(m + 1) * ntiles] bin-major (frame_table_at)
  uint64_t* tile_bytes;
  uint64_t* pre_cnt;                       // ... their exclusive prefixes over the tiles of a bin
  uint64_t* pre_bytes;
  uint64_t* totals;                        // [2 * (m + 1)] messages of every bin, then payload bytes of every bin
  // behind the totals
  int64_t* indices;                        // [n] bin c's ascending message indices start at index_base[c]
  uint64_t index_base[kFrameBins];
  uint64_t* new_offsets[kMaxFrameIds];     // class c: [count(c) + 1] offsets into out[c]
  uint8_t* out[kMaxFrameIds];              // class c's payload region (16-byte aligned)
  uint64_t* dst;                           // [n] where in out[class] a message's payload starts
};

}  // namespace rh
