// Row filters (rh_filter_*, rh_decode*_where): parameters of the filter kernel and of the compaction kernels (filter.hip),
// shared by host and device code.  Not one of the headers the specialised kernels include: the kernel-cache key does not
// see this file.
#pragma once
#include "program.h"
#include "filter_core.h"
#include "validate.h"      // VErr: one malformed record, as the validation kernel lists it

namespace rh {

constexpr uint32_t kFilterSlots = 64;      // the kept count is added per workgroup into slot (workgroup & 63): program.h kNullSlots

// rh_k_filter: rh_k_validate's walk (one lane per record, 256 records per workgroup, nothing stored or counted) that also
// evaluates the predicate's terms at the ops they mark.
struct FParams {
  const uint8_t* data;       // packed Avro payload (16-byte aligned)
  const uint64_t* offsets;   // n + 1 record offsets into data
  uint64_t data_len;
  uint64_t n;
  uint64_t rec_limit;        // only malformed records below this index are listed and counted (n = all)
  const Op* prog;            // the WRITER's plain program
  const uint32_t* sym_off;
  const uint8_t* sym_data;
  int32_t list_depth;
  uint32_t win_bytes;        // LDS bytes of the input window
  uint64_t* keep;            // [ceil(n / 64)] bit i of word w: record 64 w + i is well-formed and matches (one word per wavefront)
  uint64_t* bad;             // [ceil(n / 64)] ... is malformed
  VErr* list;                // [cap] malformed records, in no particular order
  uint32_t cap;
  uint32_t pad;
  unsigned long long* count; // [0] exact number of malformed records below rec_limit (zero at launch)
  unsigned long long* kept;  // [kFilterSlots] kept records, summed by the host (zero at launch)
  const uint8_t* cbytes;     // the byte comparands of the terms (FilterTerm::boff)
  FilterProgram flt;
};

// lengths of the kept records -> two exclusive scans (kept rank, kept bytes) -> new offsets -> gather
struct CParams {
  const uint8_t* data;
  const uint64_t* offsets;   // [n + 1]
  uint64_t n;
  const uint64_t* keep;      // FParams::keep
  uint32_t nblocks;          // ceil(n / kFilterBlock)
  uint32_t pad;
  uint64_t* blockcnt;        // [nblocks] kept records of every workgroup, then their exclusive prefix (in place)
  uint64_t* blockbytes;      // [nblocks] kept bytes likewise
  uint64_t* wordrank;        // [ceil(n / 64)] kept records in front of every keep word
  uint64_t* new_offsets;     // [kept + 1]
  uint8_t* out;              // compacted payload (16-byte aligned)
};

}  // namespace rh
