// CDNA4 (gfx950) kernels of the framed-message join (rh_join_*): the datums of several encode results put into
// message order with a Confluent or single-object header stamped in front of each, a stable multi-way merge and a ragged byte
// gather over the whole output -- the mirror of frame.hip.
//
//   rh_k_join_lengths     one lane per source row, 256 per workgroup: its source by a search of the source table (device memory,
//                         a uniform number of turns), the message it becomes (indices[r], or r), that message's length (header +
//                         datum), the datum's address and the source.  With indices the position is claimed by one atomic OR in a
//                         bitmap; the lowest out-of-range row and the lowest position claimed twice are kept by 64-bit atomicMins
//                         that only offending lanes issue.
//   rh_k_join_tile_sums   one workgroup per 256 messages: the bytes of the tile.
//   rh_k_join_scan        one workgroup: the exclusive prefix of the tile sums, 256 tiles a round with a carry, and the total.
//   rh_k_join_offsets     one workgroup per tile: the 64-bit exclusive prefix of the message lengths, and the base of every chunk
//                         that a message of the tile opens.  The host reads the bases, checks the 32-bit limit, leases the result.
//   rh_k_join_gather      one wavefront per 64 messages, 16 lanes per message: the message's i32 offset in its chunk, the header
//                         bytes, then the datum, 16-byte stores aligned on the destination fed by unaligned loads that stay inside
//                         the datum, single bytes at the ragged ends.
// Plain C++, vector stores only.  Every loop with a cross-lane step (shuffle, barrier) runs over all lanes of the wavefront or the
// workgroup with a uniform trip count.  frame_join_core.h states the arithmetic; tools/frame_join_check.cpp runs
// these steps in this order on the CPU.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frame_join.h"

namespace rh {

typedef uint32_t jn_v4 __attribute__((ext_vector_type(4)));
typedef jn_v4 __attribute__((aligned(1))) jn_v4u;

extern "C" __global__ void __launch_bounds__(kJoinTile) rh_k_join_lengths(JoinParams J) {
  const uint64_t r = (uint64_t)blockIdx.x * kJoinTile + threadIdx.x;
  if (r >= J.n) return;      // (no cross-lane step below)
  const FrameDesc d = frame_desc(J.kind);
  const uint32_t s = join_source_of(J.src, J.nsrc, r, J.turns);
  const JoinSource S = J.src[s];
  const uint64_t j = join_row_in_source(J.src, s, r);
  const int64_t o0 = S.off[j], o1 = S.off[j + 1];
  if (o0 < 0 || o1 < o0 || (uint64_t)o1 > S.data_bytes) {
    atomicMin(&J.ctrl[kJoinBadSource], (unsigned long long)r);
    return;
  }
  uint64_t p = r;
  if (J.indices) {
    const int64_t v = J.indices[r];
    if (!join_in_range(v, J.n)) {
      atomicMin(&J.ctrl[kJoinBadRange], (unsigned long long)r);
      return;
    }
    p = (uint64_t)v;
    const uint32_t bit = join_claim_bit(p);
    if (atomicOr(&J.claim[join_claim_word(p)], bit) & bit) atomicMin(&J.ctrl[kJoinBadTwice], (unsigned long long)p);
  }
  J.len[p] = d.header + (uint32_t)(o1 - o0);
  J.who[p] = s;
  J.at[p] = (uint64_t)reinterpret_cast<uintptr_t>(S.data + o0);
}

// --------------------------------------------------------------------------
// prefix sums
// --------------------------------------------------------------------------
__device__ __forceinline__ uint64_t jn_wave_incl_scan64(uint64_t v, uint32_t lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t up = __shfl_up(v, d, 64);
    if ((int)lane >= d) v += up;
  }
  return v;
}

// the workgroup's inclusive prefix of v and, in *total, the workgroup's sum; wt: 4 words of LDS.  Every lane calls it.
__device__ __forceinline__ uint64_t jn_block_incl_scan64(uint64_t v, uint64_t* wt, uint64_t* total) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t incl = jn_wave_incl_scan64(v, lane);
  __syncthreads();                       // (wt may still be read from the previous round)
  if (lane == 63) wt[wave] = incl;
  __syncthreads();
  uint64_t before = 0;
  for (uint32_t w = 0; w < wave; w++) before += wt[w];
  *total = wt[0] + wt[1] + wt[2] + wt[3];
  return before + incl;
}

extern "C" __global__ void __launch_bounds__(kJoinTile) rh_k_join_tile_sums(JoinParams J) {
  __shared__ uint64_t wt[4];
  const uint64_t p = (uint64_t)blockIdx.x * kJoinTile + threadIdx.x;
  const uint64_t v = p < J.n ? J.len[p] : 0;
  uint64_t total;
  (void)jn_block_incl_scan64(v, wt, &total);
  if (threadIdx.x == 0) J.tile_sum[blockIdx.x] = total;
}

extern "C" __global__ void __launch_bounds__(kJoinTile) rh_k_join_scan(JoinParams J) {
  __shared__ uint64_t wt[4];
  uint64_t carry = 0;
  for (uint64_t base = 0; base < J.ntiles; base += kJoinTile) {      // (uniform over the workgroup)
    const uint64_t t = base + threadIdx.x;
    const uint64_t v = t < J.ntiles ? J.tile_sum[t] : 0;
    uint64_t total;
    const uint64_t incl = jn_block_incl_scan64(v, wt, &total);
    if (t < J.ntiles) J.tile_pre[t] = carry + incl - v;
    carry += total;
  }
  if (threadIdx.x == 0) {
    J.abs[J.n] = carry;
    J.ctrl[kJoinCtrlWords + J.k] = carry;
  }
}

extern "C" __global__ void __launch_bounds__(kJoinTile) rh_k_join_offsets(JoinParams J) {
  __shared__ uint64_t wt[4];
  const uint64_t p = (uint64_t)blockIdx.x * kJoinTile + threadIdx.x;
  const uint64_t v = p < J.n ? J.len[p] : 0;
  uint64_t total;
  const uint64_t incl = jn_block_incl_scan64(v, wt, &total);
  if (p < J.n) {
    const uint64_t a = J.tile_pre[blockIdx.x] + incl - v;
    J.abs[p] = a;
    if (join_opens_chunk(p, J.sz, J.k)) J.ctrl[kJoinCtrlWords + p / J.sz] = a;
  }
}

// --------------------------------------------------------------------------
// gather
// --------------------------------------------------------------------------
// one message by the kFrameGroup lanes of one group: the header, then `len` datum bytes from s (join_copy_plan); no cross-lane step
__device__ __forceinline__ void jn_group_message(uint8_t* dst, const uint8_t* s, uint64_t len, uint64_t id, const FrameDesc& d, uint32_t sub) {
  if (sub < d.header) dst[sub] = join_header_byte(d, id, sub);
  if (!len) return;
  const FrameCopy c = join_copy_plan((uint64_t)reinterpret_cast<uintptr_t>(dst), d, len);
  uint8_t* const o = dst + d.header;
  if (sub < c.head) o[sub] = s[sub];
  const uint8_t* const sb = s + c.head;
  uint8_t* const db = o + c.head;
  for (uint64_t v = sub; v < c.nvec; v += kFrameGroup) {
    const jn_v4 x = *reinterpret_cast<const jn_v4u*>(sb + (v << 4));
    *reinterpret_cast<jn_v4*>(db + (v << 4)) = x;
  }
  const uint64_t done = c.head + (c.nvec << 4);
  if (sub < c.tail) o[done + sub] = s[done + sub];
}

extern "C" __global__ void __launch_bounds__(kJoinTile) rh_k_join_gather(JoinParams J) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t r0 = ((uint64_t)blockIdx.x * (kJoinTile / 64) + (threadIdx.x >> 6)) << 6;      // this wavefront's first message
  if (r0 >= J.n) return;                                                                         // (the whole wavefront)
  const FrameDesc d = frame_desc(J.kind);
  const uint64_t p = r0 + lane;
  // lane j holds message r0 + j: where its datum is, how long, whose id, where the message goes (0: no message)
  uint64_t src = 0, len = 0, dst = 0, id = 0;
  if (p < J.n) {
    const uint32_t c = join_chunk_of(p, J.sz, J.k);
    const uint64_t base = J.ctrl[kJoinCtrlWords + c];
    const uint64_t a = J.abs[p];
    int32_t* const off = reinterpret_cast<int32_t*>(J.outptr[2 * c]);
    const uint64_t row = p - join_chunk_start(c, J.sz);
    off[row] = (int32_t)(a - base);
    if (join_closes_chunk(p, J.n, J.sz, J.k)) off[row + 1] = (int32_t)(J.abs[p + 1] - base);
    src = J.at[p];
    len = (uint64_t)J.len[p] - d.header;
    id = J.src[J.who[p]].id;
    dst = (uint64_t)reinterpret_cast<uintptr_t>(reinterpret_cast<uint8_t*>(J.outptr[2 * c + 1]) + (a - base));
  }
  const uint32_t group = lane / kFrameGroup, sub = lane % kFrameGroup;
  for (uint32_t k = 0; k < kFrameRounds; k++) {      // (every lane runs every round: the shuffles are over the whole wavefront)
    const int j = (int)(kFrameGroups * k + group);
    const uint64_t sj = __shfl(src, j, 64), lj = __shfl(len, j, 64), dj = __shfl(dst, j, 64), ij = __shfl(id, j, 64);
    if (dj) jn_group_message(reinterpret_cast<uint8_t*>((uintptr_t)dj), reinterpret_cast<const uint8_t*>((uintptr_t)sj), lj, ij, d, sub);
  }
}

}  // namespace rh

// --------------------------------------------------------------------------
// launchers (engine_frame_join.cpp)
// --------------------------------------------------------------------------
// J->ctrl holds kJoinNone in its first kJoinCtrlWords words and J->claim is zero: lengths, then the three prefix steps
extern "C" int rh_launch_join_lengths(const rh::JoinParams* J, void* stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(rh::rh_k_join_lengths, dim3((uint32_t)J->ntiles), dim3(rh::kJoinTile), 0, (hipStream_t)stream, *J);
  return (int)hipGetLastError();
}

extern "C" int rh_launch_join_scan(const rh::JoinParams* J, void* stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(rh::rh_k_join_tile_sums, dim3((uint32_t)J->ntiles), dim3(rh::kJoinTile), 0, (hipStream_t)stream, *J);
  hipLaunchKernelGGL(rh::rh_k_join_scan, dim3(1), dim3(rh::kJoinTile), 0, (hipStream_t)stream, *J);
  hipLaunchKernelGGL(rh::rh_k_join_offsets, dim3((uint32_t)J->ntiles), dim3(rh::kJoinTile), 0, (hipStream_t)stream, *J);
  return (int)hipGetLastError();
}

extern "C" int rh_launch_join_gather(const rh::JoinParams* J, void* stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(rh::rh_k_join_gather, dim3((uint32_t)J->ntiles), dim3(rh::kJoinTile), 0, (hipStream_t)stream, *J);
  return (int)hipGetLastError();
}
