// CDNA4 (gfx950) kernels of the framed-message split (rh_frame_*): Kafka-framed Avro -- Confluent wire format or
// Avro single-object encoding -- checked, partitioned by writer schema id and stripped of its headers, a stable multi-way
// partition and a ragged byte gather over the whole input.
//
//   rh_k_frame_classify   one lane per message, 256 per workgroup: the header read byte by byte from global memory (its start is
//                         unaligned; nothing past the message's end is read), one verdict byte per message, the tile's message
//                         and payload-byte counts per bin through an LDS histogram, the lowest failing index by one 64-bit
//                         atomicMin that only failing lanes issue.
//   rh_k_frame_scan       one workgroup per (bin, table): the exclusive prefix of the bin's tile counts / tile bytes over the
//                         tiles, 256 tiles a round with a carry, and the bin's total.
//   rh_k_frame_offsets    per tile and per bin the tile's table says is present: the stable rank and the byte prefix of the bin's
//                         messages -> indices, new_offsets (relative to the bin's own region) and every message's destination.
//   rh_k_frame_gather     one wavefront per 64 messages, 16 lanes per message: the payload (the message minus its header) copied to
//                         its place, 16-byte stores aligned on the destination, bytes at the ragged ends.  Neighbours of one
//                         class are not contiguous in the source -- a header lies between them -- so nothing is merged.
// Plain C++, vector stores only.  Every loop with a cross-lane step (ballot, shuffle, barrier) runs over all lanes of the wavefront
// or the workgroup with a uniform trip count.  frame_core.h states the arithmetic; tools/frame_check.cpp runs
// these steps in this order on the CPU.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frame.h"

namespace rh {

typedef uint32_t fr_v4 __attribute__((ext_vector_type(4)));
typedef fr_v4 __attribute__((aligned(1))) fr_v4u;

extern "C" __global__ void __launch_bounds__(kFrameTile) rh_k_frame_classify(FrameParams F) {
  __shared__ uint64_t s_ids[kMaxFrameIds];
  __shared__ uint32_t h_cnt[kFrameBins];
  __shared__ unsigned long long h_bytes[kFrameBins];
  const uint32_t tid = threadIdx.x;
  if (tid < kMaxFrameIds) s_ids[tid] = tid < F.m ? F.ids[tid] : ~0ull;
  if (tid < kFrameBins) { h_cnt[tid] = 0; h_bytes[tid] = 0; }
  __syncthreads();
  const uint64_t i = (uint64_t)blockIdx.x * kFrameTile + tid;
  const FrameDesc d = frame_desc(F.kind);
  if (i < F.n) {
    const uint64_t b = F.offsets[i], e = F.offsets[i + 1];
    // (offsets that run backwards or past the payload -- a device caller's -- read as a message too short to hold a header)
    const uint8_t v = (b <= e && e <= F.data_len) ? frame_verdict(F.data, b, e, d, s_ids, F.m) : kFrameShort;
    F.cls[i] = v;
    const uint32_t bin = frame_bin(v, F.m);
    if (bin > F.m || (bin == F.m && !F.skip_unknown)) {
      atomicMin(F.first_bad, (unsigned long long)i);
    } else {
      atomicAdd(&h_cnt[bin], 1u);
      const uint64_t len = frame_payload_len(b, e, bin, F.m, d);
      if (len) atomicAdd(&h_bytes[bin], (unsigned long long)len);
    }
  }
  __syncthreads();
  if (tid <= F.m) {
    const uint64_t at = frame_table_at(F.ntiles, tid, blockIdx.x);
    F.tile_cnt[at] = h_cnt[tid];
    F.tile_bytes[at] = h_bytes[tid];
  }
}

// --------------------------------------------------------------------------
// prefix sums
// --------------------------------------------------------------------------
__device__ __forceinline__ uint64_t fr_wave_incl_scan64(uint64_t v, uint32_t lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t up = __shfl_up(v, d, 64);
    if ((int)lane >= d) v += up;
  }
  return v;
}

// one workgroup per (bin, table): blockIdx.x = 2 * bin + table (0 = messages, 1 = payload bytes)
extern "C" __global__ void __launch_bounds__(kFrameTile) rh_k_frame_scan(FrameParams F) {
  __shared__ uint64_t wt[4];
  const uint32_t bin = blockIdx.x >> 1, which = blockIdx.x & 1;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t* const in = (which ? F.tile_bytes : F.tile_cnt) + frame_table_at(F.ntiles, bin, 0);
  uint64_t* const out = (which ? F.pre_bytes : F.pre_cnt) + frame_table_at(F.ntiles, bin, 0);
  uint64_t carry = 0;
  for (uint64_t base = 0; base < F.ntiles; base += kFrameTile) {      // (uniform over the workgroup)
    const uint64_t t = base + threadIdx.x;
    const uint64_t v = t < F.ntiles ? in[t] : 0;
    const uint64_t incl = fr_wave_incl_scan64(v, lane);
    __syncthreads();                       // (wt may still be read from the previous round)
    if (lane == 63) wt[wave] = incl;
    __syncthreads();
    uint64_t before = 0;
    for (uint32_t w = 0; w < wave; w++) before += wt[w];
    if (t < F.ntiles) out[t] = carry + before + incl - v;
    carry += wt[0] + wt[1] + wt[2] + wt[3];
  }
  if (threadIdx.x == 0) F.totals[which * (F.m + 1) + bin] = carry;
}

extern "C" __global__ void __launch_bounds__(kFrameTile) rh_k_frame_offsets(FrameParams F) {
  __shared__ uint32_t wc[4];
  __shared__ uint64_t wb[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t tile = blockIdx.x;
  const uint64_t i = tile * kFrameTile + tid;
  const FrameDesc d = frame_desc(F.kind);
  uint32_t bin = F.m + 1;      // (a lane past n is in no bin)
  uint64_t len = 0;
  if (i < F.n) {
    bin = frame_bin(F.cls[i], F.m);
    len = frame_payload_len(F.offsets[i], F.offsets[i + 1], bin, F.m, d);
  }
  for (uint32_t c = 0; c <= F.m; c++) {
    const uint64_t at = frame_table_at(F.ntiles, c, tile);
    if (F.tile_cnt[at] == 0) continue;                      // (the same word for every lane of the workgroup: uniform)
    const bool mine = bin == c;
    const uint64_t bal = __ballot(mine);
    const uint32_t r_wave = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    const uint64_t q_incl = fr_wave_incl_scan64(mine ? len : 0ull, lane);
    __syncthreads();                       // (wc / wb may still be read from the previous bin)
    if (lane == 63) { wc[wave] = (uint32_t)__popcll(bal); wb[wave] = q_incl; }
    __syncthreads();
    uint32_t r0 = 0;
    uint64_t q0 = 0;
    for (uint32_t w = 0; w < wave; w++) { r0 += wc[w]; q0 += wb[w]; }
    if (mine) {
      const uint64_t rank = frame_rank(F.pre_cnt[at], (uint64_t)r0 + r_wave);
      const uint64_t byte = frame_byte(F.pre_bytes[at], q0 + q_incl - len);
      F.indices[F.index_base[c] + rank] = (int64_t)i;
      if (c < F.m) {
        F.new_offsets[c][rank] = byte;
        F.dst[i] = byte;
      }
    }
  }
  // the closing entry of every class's offsets
  if (blockIdx.x == 0 && tid < F.m) F.new_offsets[tid][F.totals[tid]] = F.totals[F.m + 1 + tid];
}

// --------------------------------------------------------------------------
// gather
// --------------------------------------------------------------------------
// `len` bytes from s to d by the kFrameGroup lanes of one group (frame_copy_plan); no cross-lane step
__device__ __forceinline__ void fr_group_copy(uint8_t* d, const uint8_t* s, uint64_t len, uint32_t sub) {
  const FrameCopy c = frame_copy_plan((uint64_t)reinterpret_cast<uintptr_t>(d), len);
  if (sub < c.head) d[sub] = s[sub];
  const uint8_t* const sb = s + c.head;
  uint8_t* const db = d + c.head;
  for (uint64_t v = sub; v < c.nvec; v += kFrameGroup) {
    const fr_v4 x = *reinterpret_cast<const fr_v4u*>(sb + (v << 4));
    *reinterpret_cast<fr_v4*>(db + (v << 4)) = x;
  }
  const uint64_t done = c.head + (c.nvec << 4);
  if (sub < c.tail) d[done + sub] = s[done + sub];
}

extern "C" __global__ void __launch_bounds__(kFrameTile) rh_k_frame_gather(FrameParams F) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t r0 = ((uint64_t)blockIdx.x * (kFrameTile / 64) + (threadIdx.x >> 6)) << 6;      // this wavefront's first message
  if (r0 >= F.n) return;                                                                          // (the whole wavefront)
  const FrameDesc d = frame_desc(F.kind);
  const uint64_t i = r0 + lane;
  // lane j holds message r0 + j: where its payload is, how long, where it goes
  uint64_t src = 0, len = 0, dst = 0;
  if (i < F.n) {
    const uint32_t v = F.cls[i];
    if (v < F.m) {
      const uint64_t b = F.offsets[i];
      src = (uint64_t)reinterpret_cast<uintptr_t>(F.data + b + d.header);
      len = (F.offsets[i + 1] - b) - d.header;
      dst = (uint64_t)reinterpret_cast<uintptr_t>(F.out[v] + F.dst[i]);
    }
  }
  const uint32_t group = lane / kFrameGroup, sub = lane % kFrameGroup;
  for (uint32_t k = 0; k < kFrameRounds; k++) {      // (every lane runs every round: the shuffles are over the whole wavefront)
    const int j = (int)(kFrameGroups * k + group);
    const uint64_t sj = __shfl(src, j, 64), lj = __shfl(len, j, 64), dj = __shfl(dst, j, 64);
    if (lj) fr_group_copy(reinterpret_cast<uint8_t*>((uintptr_t)dj), reinterpret_cast<const uint8_t*>((uintptr_t)sj), lj, sub);
  }
}

}  // namespace rh

// --------------------------------------------------------------------------
// launchers (engine_frame.cpp)
// --------------------------------------------------------------------------
// verdicts, tile tables, the lowest failing index (F->first_bad holds kFrameNoFailure), then the prefixes and the totals
extern "C" int rh_launch_frame_classify(const rh::FrameParams* F, void* stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(rh::rh_k_frame_classify, dim3((uint32_t)F->ntiles), dim3(rh::kFrameTile), 0, (hipStream_t)stream, *F);
  return (int)hipGetLastError();
}

extern "C" int rh_launch_frame_scan(const rh::FrameParams* F, void* stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(rh::rh_k_frame_scan, dim3(2 * (F->m + 1)), dim3(rh::kFrameTile), 0, (hipStream_t)stream, *F);
  return (int)hipGetLastError();
}

extern "C" int rh_launch_frame_offsets(const rh::FrameParams* F, void* stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(rh::rh_k_frame_offsets, dim3((uint32_t)F->ntiles), dim3(rh::kFrameTile), 0, (hipStream_t)stream, *F);
  return (int)hipGetLastError();
}

extern "C" int rh_launch_frame_gather(const rh::FrameParams* F, void* stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(rh::rh_k_frame_gather, dim3((uint32_t)F->ntiles), dim3(rh::kFrameTile), 0, (hipStream_t)stream, *F);
  return (int)hipGetLastError();
}
