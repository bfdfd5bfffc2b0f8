// Tolerant decode (rh_validate*, rh_decode*_tolerant): parameters of the validation kernel and of the patch kernels
// (validate.hip), shared by host and device code.  Not one of the headers the specialised kernels include: the
// kernel-cache key does not see this file.
#pragma once
#include "program.h"

namespace rh {

// One malformed record: what report_errors keeps for the lowest erroring lane of a tile only, kept for every lane.
struct VErr {
  uint64_t rec;      // record index inside the launch
  uint32_t code;     // ErrCode
  uint32_t pad;
  int64_t detail;
};

// rh_k_validate: one lane per record, 256 records per workgroup, the careful walk with nothing stored or counted.
struct VParams {
  const uint8_t* data;       // packed Avro payload (16-byte aligned)
  const uint64_t* offsets;   // n + 1 record offsets into data
  uint64_t data_len;
  uint64_t n;
  uint64_t rec_limit;        // only malformed records below this index are listed and counted (n = all)
  const Op* prog;
  const uint32_t* sym_off;
  const uint8_t* sym_data;
  int32_t list_depth;
  uint32_t win_bytes;        // LDS bytes of the input window
  uint64_t* bitmap;          // [ceil(n / 64)] bit i of word w: record 64 w + i is malformed (one word per wavefront)
  VErr* list;                // [cap] malformed records, in no particular order
  uint32_t cap;
  unsigned long long* count; // [0] exact number of malformed records below rec_limit (zero at launch)
};

// The patch kernels: new record lengths (placeholder for malformed records) -> exclusive scan -> gather.
constexpr uint32_t kPatchBlock = 256;     // records per workgroup of the length / offset kernels
struct GParams {
  const uint8_t* data;
  const uint64_t* offsets;   // [n + 1]
  uint64_t n;
  const uint64_t* bitmap;    // VParams::bitmap
  const uint8_t* ph;         // the placeholder datum (device copy)
  uint32_t ph_len;
  uint32_t nblocks;          // ceil(n / kPatchBlock)
  uint64_t* blocksum;        // [nblocks] bytes of every workgroup's records, then their exclusive prefix (in place)
  uint64_t* new_offsets;     // [n + 1]
  uint8_t* out;              // patched payload (16-byte aligned)
};

}  // namespace rh
