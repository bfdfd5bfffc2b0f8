// Deflate blocks written on the device (rh_deflate_blocks): parameters of the two kernels of deflate.hip,
// shared by host and device code.  Not one of the headers the specialised kernels include.
#pragma once
#include "deflate_core.h"

namespace rh {

constexpr uint32_t kSegLast = 1u << 31;      // DeflateParams::seg_len: the segment is the last of its stream

// rh_k_deflate: one wavefront per segment (a workgroup of 64), segments dealt grid-stride.
struct DeflateParams {
  const uint8_t* data;          // the uploaded payloads
  uint64_t data_len;            // readable bytes at data
  const uint64_t* seg_in;       // [ns] where the segment's input starts in data
  const uint32_t* seg_len;      // [ns] its bytes (<= rhd::kSegment) | kSegLast
  const uint64_t* slot;         // [ns] where its output goes in scratch: a multiple of 16, rhd::segment_bound bytes at least
  uint8_t* scratch;
  uint64_t scratch_len;         // writable bytes at scratch
  uint32_t* seg_size;           // [ns] out: the bytes written into the slot
  uint32_t ns;
  uint32_t strategy;            // rhd::AUTO .. rhd::DYNAMIC
  unsigned long long* bad;      // [0] ~(lowest segment whose table entry or whose writer was refused), 0 if none
};

// rh_k_deflate_gather: segment s's seg_size[s] bytes from scratch + slot[s] to out + out_at[s].
struct DeflateGatherParams {
  const uint8_t* scratch;
  uint64_t scratch_len;
  const uint64_t* slot;         // [ns]
  const uint32_t* seg_size;     // [ns]
  const uint64_t* out_at;       // [ns]
  uint8_t* out;
  uint64_t out_len;             // writable bytes at out
  uint32_t ns;
  uint32_t pad;
  unsigned long long* bad;
};

}  // namespace rh
