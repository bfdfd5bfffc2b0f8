// Deflate blocks on the device (rh_decode_cblocks / rh_inflate_blocks): parameters of the two kernels of
// inflate.hip, shared by host and device code.  Not one of the headers the specialised kernels include.
#pragma once
#include "inflate_core.h"

namespace rh {

// rh_k_inflate_size and rh_k_inflate_emit: one wavefront per container block (a workgroup of 64), blocks dealt grid-stride.
struct InflateParams {
  const uint8_t* data;          // the uploaded file: compressed payloads at [start[b], end[b])
  uint64_t data_len;            // readable bytes at data
  const uint64_t* start;        // [nb]
  const uint64_t* end;          // [nb]
  uint32_t nb;
  uint32_t pad;
  uint64_t max_out;             // a block that inflates to this much or more is ST_TOO_LARGE
  uint64_t* size;               // [nb] size pass: out (the bytes counted until the walk stopped); emit pass: in
  rhi::Status* status;          // [nb] size pass: out; emit pass: in (a block whose code is not ST_OK is left alone)
  const uint64_t* out_start;    // [nb] emit pass: block b's bytes go to out[out_start[b] .. out_start[b] + size[b])
  uint8_t* out;
  uint64_t out_len;             // writable bytes at out
  unsigned long long* emit_bad; // [0] emit pass: ~(lowest block whose walk disagreed with its size pass), 0 if none
};

}  // namespace rh
