// CDNA4 (gfx950) kernels that inflate the deflate blocks of a container on the device (rh_decode_cblocks, rh_inflate_blocks;
// DESIGN.md 14, "Deflate blocks on the device").
//
//   rh_k_inflate_size   walks every block's raw-deflate stream (inflate_core.h) and writes its inflated size, counted in 64
//                       bits, and its verdict.  Nothing else is stored: a match needs no history to be counted.
//   rh_k_inflate_emit   walks the streams the size pass accepted again and writes their bytes at out_start[b].
//
// One wavefront per container block, a workgroup of exactly one wavefront.  ALL 64 lanes run the same walk over the same input:
// the serial decode costs a wavefront what it costs a lane, every value is wave-uniform by construction, and the cooperative
// steps (table loads, the match copy, the flush) sit in control flow that every lane takes -- no loop here depends on which
// lanes happen to be active, and nothing is broadcast.  Lane 0 alone stores tables and literals.  The last 32 KiB of output
// live in an LDS ring; matches are copied ring to ring by all lanes, and the ring drains to global memory in 16-byte stores.
// Global memory is never read back, so no store has to be visible to another lane.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "inflate.h"

namespace rh {

constexpr uint32_t kWave = 64;
constexpr uint32_t kRing = 32768, kRingMask = kRing - 1;
constexpr uint32_t kFlushAt = 4096;      // bytes that wait in the ring at most (+ one match): far from the 32 KiB that overwrite them

// The sink of the emit walk.  Byte i of the block's output sits at ring[(i + skew) & kRingMask], skew = the low 4 bits of its
// global address: a 16-byte-aligned global store reads a 16-byte-aligned piece of the ring that never straddles the wrap.
// Every store to global memory is inside [g, g + size): n <= size is checked before n grows, and flush_to never passes n.
struct RingSink {
  uint8_t* ring;
  uint8_t* g;             // where byte 0 of this block goes
  uint64_t size;          // what the size pass counted
  uint64_t n, flushed;
  uint32_t skew, lane;

  __device__ __forceinline__ uint64_t produced() const { return n; }
  __device__ __forceinline__ uint32_t slot(uint64_t i) const { return ((uint32_t)i + skew) & kRingMask; }

  __device__ __forceinline__ void flush_to(uint64_t to) {      // flushed <= to <= n
    __syncthreads();
    uint64_t a = flushed;
    const uint32_t mis = slot(a) & 15;
    if (mis && a < to) {      // up to the first 16-byte boundary of global memory, byte by byte
      const uint64_t left = to - a;
      const uint32_t head = left < 16 - mis ? (uint32_t)left : 16 - mis;
      if (lane < head) g[a + lane] = ring[slot(a + lane)];
      a += head;
    }
    const uint64_t nvec = (to - a) >> 4;
    for (uint64_t v = lane; v < nvec; v += kWave) {
      const uint4 x = *reinterpret_cast<const uint4*>(ring + slot(a + 16 * v));
      *reinterpret_cast<uint4*>(g + a + 16 * v) = x;
    }
    a += nvec << 4;
    if (lane < (uint32_t)(to - a)) g[a + lane] = ring[slot(a + lane)];      // (fewer than 16 are left)
    flushed = to;
    __syncthreads();      // (the ring's loads are done before anything overwrites it)
  }
  __device__ __forceinline__ void maybe_flush() {
    if (n - flushed >= kFlushAt) flush_to(n - (slot(n) & 15));
  }

  __device__ __forceinline__ bool lit(uint8_t v) {
    if (n >= size) return false;
    if (lane == 0) ring[slot(n)] = v;
    n++;
    maybe_flush();
    return true;
  }
  // Byte i of the match is byte (i mod dist) of the last dist bytes: every source is older than the match, so the lanes need
  // no order among themselves, for dist < length too.  In a ring of exactly 32 KiB the slot of byte n + i is the slot of byte
  // n + i - 32768, which is a SOURCE of this match only for a lane index that is not above i (dist <= 32768): it is loaded in
  // the same or an earlier turn of the loop, and within a turn every lane's load comes before any lane's store.
  __device__ __forceinline__ bool copy(uint32_t length, uint32_t dist) {
    if (length > size - n) return false;
    __syncthreads();
    for (uint32_t i = lane; i < length; i += kWave) {
      const uint32_t back = dist >= length ? i : i % dist;
      const uint8_t v = ring[slot(n - dist + back)];
      ring[slot(n + i)] = v;
    }
    n += length;
    maybe_flush();
    return true;
  }
  __device__ __forceinline__ bool stored(const uint8_t* src, uint32_t k) {
    if (k > size - n) return false;
    while (k) {
      const uint32_t c = k < kFlushAt ? k : kFlushAt;
      __syncthreads();
      for (uint32_t i = lane; i < c; i += kWave) ring[slot(n + i)] = src[i];
      n += c; src += c; k -= c;
      maybe_flush();
    }
    return true;
  }
};

extern "C" __global__ void __launch_bounds__(kWave) rh_k_inflate_size(InflateParams P) {
  __shared__ rhi::Tables T;
  const bool writer = threadIdx.x == 0;
  for (uint64_t b = blockIdx.x; b < (uint64_t)P.nb; b += gridDim.x) {
    const uint64_t st = P.start[b], en = P.end[b];
    __syncthreads();
    if (writer) T.fixed_ready = 0;
    __syncthreads();
    rhi::CountSink sink;
    rhi::Status s = rhi::status(rhi::ST_INTERNAL);
    if (st <= en && en <= P.data_len) s = rhi::inflate_stream(P.data + st, en - st, T, sink, P.max_out, writer);
    if (writer) { P.size[b] = sink.n; P.status[b] = s; }
  }
}

extern "C" __global__ void __launch_bounds__(kWave) rh_k_inflate_emit(InflateParams P) {
  __shared__ __attribute__((aligned(16))) uint8_t ring[kRing];
  __shared__ rhi::Tables T;
  const bool writer = threadIdx.x == 0;
  for (uint64_t b = blockIdx.x; b < (uint64_t)P.nb; b += gridDim.x) {
    if (P.status[b].code != rhi::ST_OK) continue;      // (wave-uniform)
    const uint64_t st = P.start[b], en = P.end[b], size = P.size[b], at = P.out_start[b];
    bool ok = st <= en && en <= P.data_len && at <= P.out_len && size <= P.out_len - at;
    if (ok) {
      __syncthreads();
      if (writer) T.fixed_ready = 0;
      __syncthreads();
      RingSink sink;
      sink.ring = ring; sink.g = P.out + at; sink.size = size; sink.n = 0; sink.flushed = 0;
      sink.skew = (uint32_t)(reinterpret_cast<uintptr_t>(P.out + at) & 15); sink.lane = threadIdx.x;
      const rhi::Status s = rhi::inflate_stream(P.data + st, en - st, T, sink, P.max_out, writer);
      sink.flush_to(sink.n);
      ok = s.code == rhi::ST_OK && sink.n == size;
    }
    if (!ok && writer) atomicMax(P.emit_bad, ~(unsigned long long)b);
  }
}

}  // namespace rh

// --------------------------------------------------------------------------
// launchers (engine_container.cpp)
// --------------------------------------------------------------------------
static uint32_t inflate_grid(uint32_t nb) { return nb < (1u << 20) ? nb : (1u << 20); }

extern "C" int rh_launch_inflate_size(const rh::InflateParams* P, void* stream) {
  (void)hipGetLastError();
  if (P->nb == 0) return 0;
  hipLaunchKernelGGL(rh::rh_k_inflate_size, dim3(inflate_grid(P->nb)), dim3(rh::kWave), 0, (hipStream_t)stream, *P);
  return (int)hipGetLastError();
}

extern "C" int rh_launch_inflate_emit(const rh::InflateParams* P, void* stream) {
  (void)hipGetLastError();
  if (P->nb == 0) return 0;
  hipLaunchKernelGGL(rh::rh_k_inflate_emit, dim3(inflate_grid(P->nb)), dim3(rh::kWave), 0, (hipStream_t)stream, *P);
  return (int)hipGetLastError();
}
