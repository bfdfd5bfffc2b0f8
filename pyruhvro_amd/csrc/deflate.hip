// CDNA4 (gfx950) kernels that deflate the blocks of a container on the device (rh_deflate_blocks; DESIGN.md 14.3, "Deflate
// blocks written on the device").
//
//   rh_k_deflate          compresses every segment (deflate_core.h: at most 32 KiB of one payload) into its slot of the scratch
//                         buffer and writes the segment's size.
//   rh_k_deflate_gather   copies the segments back to back once the host has prefix-summed the sizes: the streams as they
//                         go into the file, and the download is the compressed bytes only.
//
// One wavefront per segment, a workgroup of exactly one wavefront.  Match finding is lane-parallel (position p + lane, the
// hash table in LDS, atomicMax keeps the highest position of a hash); the greedy pass, the histogram and the header are
// wave-uniform -- all lanes take the same control flow, lane 0 stores into the LDS tables, __syncthreads() is the fence -- and
// the code build runs on lane 0 alone between two fences.  Token bits are placed by a prefix sum of their code lengths, 64
// tokens per step, ORed into an LDS staging buffer that drains into the slot in aligned 16-byte stores.  Global memory is never
// read back.  Every read of input is inside the segment, every store inside its slot (deflate_core.h, "TERMINATION AND
// BOUNDS"); the table entries are checked against the buffers' lengths here once more.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "deflate.h"

namespace rh {

constexpr uint32_t kDeflateWave = 64;

extern "C" __global__ void __launch_bounds__(kDeflateWave) rh_k_deflate(DeflateParams P) {
  __shared__ __attribute__((aligned(16))) rhd::State S;
  const rhd::Ctx X = {threadIdx.x, kDeflateWave};
  for (uint64_t s = blockIdx.x; s < (uint64_t)P.ns; s += gridDim.x) {
    const uint64_t at = P.seg_in[s], slot = P.slot[s];
    const uint32_t word = P.seg_len[s], n = word & ~kSegLast;
    const bool last = (word & kSegLast) != 0;
    const uint64_t cap = rhd::segment_bound(n, last);
    const bool ok = n <= rhd::kSegment && at <= P.data_len && n <= P.data_len - at && slot <= P.scratch_len && cap <= P.scratch_len - slot;      // (wave-uniform)
    bool bad = !ok;
    uint64_t size = 0;
    if (ok) size = rhd::deflate_segment(S, X, P.data + at, n, last, P.strategy, P.scratch + slot, cap, &bad);
    if (threadIdx.x == 0) {
      P.seg_size[s] = bad ? 0u : (uint32_t)size;
      if (bad) atomicMax(P.bad, ~(unsigned long long)s);
    }
  }
}

// One wavefront per segment.  The destination decides the alignment: bytes up to its first 16-byte boundary, then aligned
// 16-byte stores fed by 16-byte loads at whatever alignment the source has there, then the bytes left.
extern "C" __global__ void __launch_bounds__(kDeflateWave) rh_k_deflate_gather(DeflateGatherParams P) {
  const uint32_t lane = threadIdx.x;
  for (uint64_t s = blockIdx.x; s < (uint64_t)P.ns; s += gridDim.x) {
    const uint64_t slot = P.slot[s], at = P.out_at[s], n = P.seg_size[s];
    if (!(slot <= P.scratch_len && n <= P.scratch_len - slot && at <= P.out_len && n <= P.out_len - at)) {
      if (lane == 0) atomicMax(P.bad, ~(unsigned long long)s);
      continue;
    }
    const uint8_t* src = P.scratch + slot;
    uint8_t* dst = P.out + at;
    const uint64_t mis = (16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15, head = n < mis ? n : mis;
    if (lane < head) dst[lane] = src[lane];
    const uint64_t nvec = (n - head) >> 4;
    for (uint64_t v = lane; v < nvec; v += kDeflateWave) {
      uint4 x;
      __builtin_memcpy(&x, src + head + 16 * v, 16);
      *reinterpret_cast<uint4*>(dst + head + 16 * v) = x;
    }
    const uint64_t done = head + (nvec << 4);
    if (lane < n - done) dst[done + lane] = src[done + lane];      // (fewer than 16 are left)
  }
}

}  // namespace rh

// --------------------------------------------------------------------------
// launchers (engine_container.cpp)
// --------------------------------------------------------------------------
static uint32_t deflate_grid(uint32_t ns) { return ns < (1u << 20) ? ns : (1u << 20); }

extern "C" int rh_launch_deflate(const rh::DeflateParams* P, void* stream) {
  (void)hipGetLastError();
  if (P->ns == 0) return 0;
  hipLaunchKernelGGL(rh::rh_k_deflate, dim3(deflate_grid(P->ns)), dim3(rh::kDeflateWave), 0, (hipStream_t)stream, *P);
  return (int)hipGetLastError();
}

extern "C" int rh_launch_deflate_gather(const rh::DeflateGatherParams* P, void* stream) {
  (void)hipGetLastError();
  if (P->ns == 0) return 0;
  hipLaunchKernelGGL(rh::rh_k_deflate_gather, dim3(deflate_grid(P->ns)), dim3(rh::kDeflateWave), 0, (hipStream_t)stream, *P);
  return (int)hipGetLastError();
}
