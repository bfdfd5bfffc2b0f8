// Framed messages, the write side (rh_frame_join): parameters of the kernels of frame_join.hip, shared by host and device code.
// Not one of the headers the specialised kernels include: the kernel-cache key does not see this file.
#pragma once
#include <stdint.h>
#include "frame_join_core.h"

namespace rh {

// the words the host reads in the call's one synchronisation, in front of the chunk bases
constexpr uint32_t kJoinBadRange = 0;         // the lowest source row whose index is outside 0 .. n-1
constexpr uint32_t kJoinBadTwice = 1;         // the lowest position that a second row named
constexpr uint32_t kJoinBadSource = 2;        // the lowest source row whose offsets run backwards or past the source's data
constexpr uint32_t kJoinCtrlWords = 4;

// lengths -> tile sums -> scan -> offsets -> (the host reads ctrl, checks the chunks' totals and leases the result) -> gather
struct JoinParams {
  const JoinSource* src;     // the source table (device memory)
  uint32_t nsrc;
  uint32_t turns;            // join_search_turns(nsrc)
  uint32_t kind;             // FrameKind
  uint32_t k;                // chunks of the result
  uint64_t n;                // messages = rows of all sources
  uint64_t ntiles;           // join_tiles(n)
  uint64_t sz;               // messages of every chunk but the last
  const int64_t* indices;    // [n] by source row: the message a row becomes; NULL: row r becomes message r
  uint32_t* claim;           // [join_claim_words(n)] zero at launch (only with indices)
  unsigned long long* ctrl;  // [kJoinCtrlWords] kJoinNone at launch, then [k + 1] chunk bases (the last: all bytes)
  // by message
  uint32_t* len;             // header + datum
  uint32_t* who;             // its source
  uint64_t* at;              // the address of its datum
  uint64_t* abs;             // [n + 1] the exclusive prefix of len
  uint64_t* tile_sum;        // [ntiles]
  uint64_t* tile_pre;        // [ntiles] their exclusive prefix
  // behind the synchronisation
  void* const* outptr;       // [k][2] a chunk's i32 offsets and its data
};

}  // namespace rh
