// CDNA4 (gfx950) kernels of the row filter (rh_filter_*, rh_decode*_where).
//
//   rh_k_filter          rh_k_validate's walk -- the generic interpreter's CAREFUL walk of the writer's plain program, every op run
//                        the way walk_drop.h runs a dropped field's, one lane per record, 256 records per workgroup, the tile's bytes
//                        in the LDS window or, past it, read from global memory -- that also evaluates a predicate: at an op a term
//                        marks, the lane notes its cursor, runs the op, and if it is still error-free reads the value back from the
//                        noted cursor (the handler has just bounds-checked those bytes) and applies filter_core.h's term_keeps.
//                        Out: one keep word per wavefront (a ballot), the exact kept count, and validation's error bitmap, list and
//                        count.  A malformed record is never kept.
//   rh_k_filter_lens / rh_k_filter_scan / rh_k_filter_offsets
//                        two prefix sums over the keep bits -- kept rank and kept bytes -> new_offsets[0 .. kept], and the rank
//                        in front of every keep word.
//   rh_k_filter_gather   the kept records copied to their new places: one wavefront per 64 records, every run of kept neighbours
//                        as ONE copy, 16-byte vectors aligned on the destination, bytes at the ragged ends.
// Small helpers of validate.hip (the block scan, the wavefront copy) are restated here: that file stays as it is.  The walk and the
// evaluation of a term (filter_walk, f_eval, f_varint, the program fetch) are in filter_eval.h, shared with rh_k_split_where.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define RH_DEEP 1      // as the interpreter of kernels.hip: any nesting the schema front-end accepts

#include "kernel_common.h"
#include "program.h"
#include "walk.h"
#include "walk_drop.h"
#include "filter.h"
#include "filter_eval.h"      // f_varint / f_eval / filter_walk: shared with rh_k_split_where (container.hip)

namespace rh {

// what DropCtx needs of the walk's context (validate.hip VCtx)
struct FCtx {
  static constexpr bool kWide = true;
  static constexpr bool kSkip = false;
  static constexpr bool kEnumImm = false;
  static constexpr bool kWaveCtr = false;
  static __device__ __forceinline__ bool enum_sym(int, uint32_t, uint32_t&, uint64_t&) { return false; }
  uint32_t* rem;             // LDS [depth][kBlock]
  const uint32_t* sym_off;
  const uint8_t* sym_data;
  uint32_t lrow, tid, lane;
  bool wave_live;
  __device__ __forceinline__ uint32_t& remaining(int d) const { return rem[d * kBlock + tid]; }
};

extern "C" __global__ void __launch_bounds__(kBlock) rh_k_filter(FParams F) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  __shared__ uint32_t wg_kept;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the launch as ONE chunk of n rows: geometry / stage_window / lane_init of the decode kernels apply as they are
  KParams P;
  P.data = F.data; P.offsets = F.offsets; P.data_len = F.data_len; P.n = F.n;
  P.sz = F.n; P.rows_last = F.n; P.k = 1; P.bpc = gridDim.x; P.nblocks = gridDim.x; P.win_bytes = F.win_bytes;
  const uint32_t depth = (uint32_t)(F.list_depth > 0 ? F.list_depth : 1);
  uint32_t* const rem = reinterpret_cast<uint32_t*>(smem);
  uint8_t* const win = smem + (size_t)depth * kBlock * 4;         // (a multiple of 1 KiB in front of it: 16-byte aligned)

  const Geo g = geometry<kBlock>(P, blockIdx.x);
  const uint64_t wb = F.offsets[g.rec0], we = F.offsets[g.rec0 + g.nrec];
  const uint64_t wb16 = wb & ~15ull;
  const bool fits = (we - wb16) <= (uint64_t)F.win_bytes;
  if (fits) stage_window<kBlock>(P, win, wb16, we, tid);
  for (uint32_t d = 0; d < depth; d++) rem[d * kBlock + tid] = 0;
  if (tid == 0) wg_kept = 0;
  __syncthreads();

  Lane L;
  lane_init(L, P, g, wb16, tid);
  if (L.live && (we - wb16) > 0xFFFFFFF0ull) fail(L, E_EOB);      // window beyond 32-bit cursors (as k_size)
  FCtx c;
  c.rem = rem; c.sym_off = F.sym_off; c.sym_data = F.sym_data;
  c.lrow = (uint32_t)g.lrow0 + tid; c.tid = tid; c.lane = lane; c.wave_live = (wave * 64) < g.nrec;
  const bool mine = tid < g.nrec;
  const FMarks marks = f_marks(F.flt);
  bool keep;
  if (fits) {
    const uint32_t wa = (uint32_t)(uintptr_t)(RH_LDS uint8_t*)win;
    L.cur += wa; L.end += wa;
    LdsAbsSrc src;
    keep = filter_walk(F.prog, &F.flt, marks, F.cbytes, c, src, L, mine);
  } else {
    GlobalSrc src{F.data + wb16, F.data_len - wb16};
    keep = filter_walk(F.prog, &F.flt, marks, F.cbytes, c, src, L, mine);
  }

  const uint64_t rec = g.rec0 + tid;
  const bool bad = mine && L.err != 0;
  keep = keep && mine && !bad;
  const uint64_t km = __ballot(keep);
  const uint64_t m = __ballot(bad);
  if (lane == 0 && wave * 64 < g.nrec) {
    F.keep[(g.rec0 >> 6) + wave] = km;
    F.bad[(g.rec0 >> 6) + wave] = m;
    if (km) atomicAdd(&wg_kept, (uint32_t)__popcll(km));
  }
  const bool listed = bad && rec < F.rec_limit;
  const uint64_t lm = __ballot(listed);
  if (lm) {      // (wave-uniform)
    unsigned long long base = 0;
    if (lane == (uint32_t)__builtin_ctzll(lm)) base = atomicAdd(F.count, (unsigned long long)__popcll(lm));
    base = __shfl(base, __builtin_ctzll(lm), 64);
    const unsigned long long at = base + (unsigned long long)__popcll(lm & ((1ull << lane) - 1ull));
    if (listed && at < (unsigned long long)F.cap) {
      VErr e; e.rec = rec; e.code = L.err; e.pad = 0; e.detail = L.edetail;
      F.list[at] = e;
    }
  }
  __syncthreads();
  if (tid == 0 && wg_kept) atomicAdd(F.kept + (blockIdx.x & (kFilterSlots - 1)), (unsigned long long)wg_kept);
}

// --------------------------------------------------------------------------
// compaction: kept rank and kept bytes -> offsets
// --------------------------------------------------------------------------
__device__ __forceinline__ uint64_t f_wave_incl_scan64(uint64_t v, uint32_t lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t up = __shfl_up(v, d, 64);
    if ((int)lane >= d) v += up;
  }
  return v;
}
// inclusive scan over the kFilterBlock threads of a workgroup; *total = the workgroup's sum.  Contains two barriers.
__device__ __forceinline__ uint64_t f_block_incl_scan64(uint64_t v, uint64_t* wt, uint64_t* total) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t incl = f_wave_incl_scan64(v, lane);
  __syncthreads();                       // (wt may still be read from the previous round)
  if (lane == 63) wt[wave] = incl;
  __syncthreads();
  uint64_t base = 0;
  for (uint32_t w = 0; w < wave; w++) base += wt[w];
  *total = wt[0] + wt[1] + wt[2] + wt[3];
  return base + incl;
}

extern "C" __global__ void __launch_bounds__(kFilterBlock) rh_k_filter_lens(CParams G) {
  __shared__ uint64_t wc[4], wb[4];
  const uint64_t i = (uint64_t)blockIdx.x * kFilterBlock + threadIdx.x;
  uint64_t tc, tb;
  f_block_incl_scan64(filter_kept(G.keep, G.n, i) ? 1ull : 0ull, wc, &tc);
  f_block_incl_scan64(filter_len(G.keep, G.offsets, G.n, i), wb, &tb);
  if (threadIdx.x == 0) { G.blockcnt[blockIdx.x] = tc; G.blockbytes[blockIdx.x] = tb; }
}

// one workgroup: blockcnt[] and blockbytes[] -> their exclusive prefixes, in place
extern "C" __global__ void __launch_bounds__(kFilterBlock) rh_k_filter_scan(CParams G) {
  __shared__ uint64_t wt[4];
  for (int which = 0; which < 2; which++) {
    uint64_t* const sum = which ? G.blockbytes : G.blockcnt;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < G.nblocks; base += kFilterBlock) {
      const uint32_t i = base + threadIdx.x;
      const uint64_t v = i < G.nblocks ? sum[i] : 0;
      uint64_t total;
      const uint64_t incl = f_block_incl_scan64(v, wt, &total);
      if (i < G.nblocks) sum[i] = carry + incl - v;
      carry += total;
    }
  }
}

extern "C" __global__ void __launch_bounds__(kFilterBlock) rh_k_filter_offsets(CParams G) {
  __shared__ uint64_t wc[4], wb[4];
  const uint64_t i = (uint64_t)blockIdx.x * kFilterBlock + threadIdx.x;
  const uint64_t c = filter_kept(G.keep, G.n, i) ? 1ull : 0ull;
  const uint64_t v = filter_len(G.keep, G.offsets, G.n, i);
  uint64_t tc, tb;
  const uint64_t ic = f_block_incl_scan64(c, wc, &tc);
  const uint64_t ib = f_block_incl_scan64(v, wb, &tb);
  const uint64_t bc = G.blockcnt[blockIdx.x], bb = G.blockbytes[blockIdx.x];
  if (c) G.new_offsets[bc + ic - 1] = bb + ib - v;
  if (i < G.n && (i & 63) == 0) G.wordrank[i >> 6] = bc + ic - c;
  if (i + 1 == G.n) G.new_offsets[bc + ic] = bb + ib;
}

// --------------------------------------------------------------------------
// compaction: gather
// --------------------------------------------------------------------------
// `len` bytes from s to d by one wavefront.  d and s are misaligned against each other in general: the vectors are cut where the
// DESTINATION is 16-byte aligned (aligned stores, unaligned loads), the bytes in front of the first and behind the last one go singly.
__device__ __forceinline__ void f_wave_copy(uint8_t* d, const uint8_t* s, uint64_t len, uint32_t lane) {
  const uint64_t mis = (16u - (uint32_t)(reinterpret_cast<uintptr_t>(d) & 15u)) & 15u;
  const uint64_t head = mis < len ? mis : len;
  if (lane < head) d[lane] = s[lane];
  const uint64_t nvec = (len - head) >> 4;
  const uint8_t* sb = s + head;
  uint8_t* db = d + head;
  for (uint64_t v = lane; v < nvec; v += 64) {
    const v4w x = *reinterpret_cast<const v4wu*>(sb + (v << 4));
    *reinterpret_cast<v4w*>(db + (v << 4)) = x;
  }
  const uint64_t done = head + (nvec << 4);
  if (done + lane < len) d[done + lane] = s[done + lane];         // (fewer than 16 bytes are left)
}

extern "C" __global__ void __launch_bounds__(kBlock) rh_k_filter_gather(CParams G) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t w = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);      // this wavefront's keep word
  const uint64_t r0 = w << 6;
  if (r0 >= G.n) return;
  const uint32_t cnt = G.n - r0 < 64 ? (uint32_t)(G.n - r0) : 64u;
  const uint64_t word = G.keep[w] & filter_valid_mask(G.n, w);
  const uint64_t rank0 = G.wordrank[w];
  uint32_t j = 0, b, e;
  while (filter_next_run(word, j, cnt, &b, &e)) {                  // (everything here is wave-uniform)
    const uint64_t s0 = G.offsets[r0 + b], s1 = G.offsets[r0 + e];
    f_wave_copy(G.out + G.new_offsets[rank0 + filter_rank_in_word(word, b)], G.data + s0, s1 - s0, lane);
    j = e;
  }
}

}  // namespace rh

// --------------------------------------------------------------------------
// launchers (engine_filter.cpp)
// --------------------------------------------------------------------------
extern "C" uint32_t rh_filter_lds_fixed(int list_depth) { return (uint32_t)(list_depth > 0 ? list_depth : 1) * rh::kBlock * 4; }

extern "C" int rh_launch_filter(const rh::FParams* F, uint32_t lds_bytes, void* stream) {
  (void)hipGetLastError();
  int e = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(rh::rh_k_filter), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 64);
  if (e) return e;
  const uint32_t nblocks = (uint32_t)((F->n + rh::kBlock - 1) / rh::kBlock);
  hipLaunchKernelGGL(rh::rh_k_filter, dim3(nblocks), dim3(rh::kBlock), lds_bytes, (hipStream_t)stream, *F);
  return (int)hipGetLastError();
}

// lengths, scan, offsets: new_offsets[0 .. kept] and wordrank[] are complete in stream order behind this
extern "C" int rh_launch_filter_offsets(const rh::CParams* G, void* stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(rh::rh_k_filter_lens, dim3(G->nblocks), dim3(rh::kFilterBlock), 0, (hipStream_t)stream, *G);
  hipLaunchKernelGGL(rh::rh_k_filter_scan, dim3(1), dim3(rh::kFilterBlock), 0, (hipStream_t)stream, *G);
  hipLaunchKernelGGL(rh::rh_k_filter_offsets, dim3(G->nblocks), dim3(rh::kFilterBlock), 0, (hipStream_t)stream, *G);
  return (int)hipGetLastError();
}

extern "C" int rh_launch_filter_gather(const rh::CParams* G, void* stream) {
  (void)hipGetLastError();
  const uint64_t waves = (G->n + 63) / 64;
  hipLaunchKernelGGL(rh::rh_k_filter_gather, dim3((uint32_t)((waves + 3) / 4)), dim3(rh::kBlock), 0, (hipStream_t)stream, *G);
  return (int)hipGetLastError();
}
