// CDNA4 (gfx950) kernels of the tolerant decode (rh_validate*, rh_decode*_tolerant; DESIGN.md "Tolerant decode").
//
//   rh_k_validate        the generic interpreter's CAREFUL walk with nothing stored and nothing counted: every op of the
//                        schema program runs the way walk_drop.h runs the ops of a dropped field.  One lane per record, 256
//                        records per workgroup, the tile's bytes staged into the LDS window as in k_size; a tile past the
//                        window is walked from global memory.  Where the decode kernels keep the lowest erroring lane of a
//                        tile (kernel_common.h report_errors), this one keeps EVERY erroring lane: one bitmap word per
//                        wavefront (a ballot), (record, code, detail) appended to a bounded list, the exact count.
//   rh_k_patch_lens / rh_k_patch_scan / rh_k_patch_offsets
//                        record lengths with the placeholder's in place of every malformed record's -> u64 offsets.
//   rh_k_patch_gather    the records -- the placeholder for the malformed ones -- copied to their new places: one wavefront
//                        per 64 records, every run of well-formed neighbours as ONE copy (they are contiguous in the source
//                        and in the destination), 16-byte vectors aligned on the destination, bytes at the ragged ends.
// There is no schema-specialised form of the validation walk (a follow-up): it only runs for calls that met a malformed record.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define RH_DEEP 1      // as the interpreter of kernels.hip: any nesting the schema front-end accepts

#include "kernel_common.h"
#include "program.h"
#include "walk.h"
#include "walk_drop.h"
#include "validate.h"

namespace rh {

// what DropCtx needs of the walk's context: list framing (one `remaining` word per list level and lane) and the enum symbols
struct VCtx {
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

typedef const __attribute__((address_space(4))) Op* VProgPtr;
__device__ __forceinline__ Op v_ld_op(VProgPtr p) {
  Op o;
  o.code = p->code; o.flags = p->flags; o.dom = p->dom; o.a = p->a; o.b = p->b; o.c = p->c;
  o.buf0 = p->buf0; o.buf1 = p->buf1; o.buf2 = p->buf2; o.node = p->node;
  return o;
}

// the program, every op counters-only and careful (walk_drop.h run_dropped)
template <class Src>
__device__ __forceinline__ void validate_walk(const Op* program, const VCtx& c, const Src& src, Lane& L) {
  const VProgPtr prog = reinterpret_cast<VProgPtr>(reinterpret_cast<uintptr_t>(program));
  int pc = 0;
  for (;;) {
    pc = __builtin_amdgcn_readfirstlane(pc);
    const Op op = v_ld_op(prog + pc);
    if (op.code == OP_END) return;
    int npc = op.code == OP_LIST_TAIL ? op.b : pc + 1;      // LIST_TAIL goes back to its LIST_NEXT
    if (op.code > OP_BIN) return;
    if (!run_dropped<false, true>(c, src, L, op)) npc = op.b;      // no lane has an item left: to LIST_END
    pc = npc;
  }
}

extern "C" __global__ void __launch_bounds__(kBlock) rh_k_validate(VParams V) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the launch as ONE chunk of n rows: geometry / stage_window / lane_init of the decode kernels apply as they are
  KParams P;
  P.data = V.data; P.offsets = V.offsets; P.data_len = V.data_len; P.n = V.n;
  P.sz = V.n; P.rows_last = V.n; P.k = 1; P.bpc = gridDim.x; P.nblocks = gridDim.x; P.win_bytes = V.win_bytes;
  const uint32_t depth = (uint32_t)(V.list_depth > 0 ? V.list_depth : 1);
  uint32_t* const rem = reinterpret_cast<uint32_t*>(smem);
  uint8_t* const win = smem + (size_t)depth * kBlock * 4;         // (a multiple of 1 KiB in front of it: 16-byte aligned)

  const Geo g = geometry<kBlock>(P, blockIdx.x);
  const uint64_t wb = V.offsets[g.rec0], we = V.offsets[g.rec0 + g.nrec];
  const uint64_t wb16 = wb & ~15ull;
  const bool fits = (we - wb16) <= (uint64_t)V.win_bytes;
  if (fits) stage_window<kBlock>(P, win, wb16, we, tid);
  for (uint32_t d = 0; d < depth; d++) rem[d * kBlock + tid] = 0;
  __syncthreads();

  Lane L;
  lane_init(L, P, g, wb16, tid);
  if (L.live && (we - wb16) > 0xFFFFFFF0ull) fail(L, E_EOB);      // window beyond 32-bit cursors (as k_size)
  VCtx c;
  c.rem = rem; c.sym_off = V.sym_off; c.sym_data = V.sym_data;
  c.lrow = (uint32_t)g.lrow0 + tid; c.tid = tid; c.lane = lane; c.wave_live = (wave * 64) < g.nrec;
  if (fits) {
    const uint32_t wa = (uint32_t)(uintptr_t)(RH_LDS uint8_t*)win;
    L.cur += wa; L.end += wa;
    LdsAbsSrc src;
    validate_walk(V.prog, c, src, L);
  } else {
    GlobalSrc src{V.data + wb16, V.data_len - wb16};
    validate_walk(V.prog, c, src, L);
  }

  const uint64_t rec = g.rec0 + tid;
  const bool bad = tid < g.nrec && L.err != 0;
  const uint64_t m = __ballot(bad);
  if (lane == 0 && wave * 64 < g.nrec) V.bitmap[(g.rec0 >> 6) + wave] = m;
  const bool listed = bad && rec < V.rec_limit;
  const uint64_t lm = __ballot(listed);
  if (lm) {      // (wave-uniform)
    unsigned long long base = 0;
    if (lane == (uint32_t)__builtin_ctzll(lm)) base = atomicAdd(V.count, (unsigned long long)__popcll(lm));
    base = __shfl(base, __builtin_ctzll(lm), 64);
    const unsigned long long at = base + (unsigned long long)__popcll(lm & ((1ull << lane) - 1ull));
    if (listed && at < (unsigned long long)V.cap) {
      VErr e; e.rec = rec; e.code = L.err; e.pad = 0; e.detail = L.edetail;
      V.list[at] = e;
    }
  }
}

// --------------------------------------------------------------------------
// patch: lengths -> offsets
// --------------------------------------------------------------------------
__device__ __forceinline__ uint64_t patched_len(const GParams& G, uint64_t i) {
  if (i >= G.n) return 0;
  const bool bad = (G.bitmap[i >> 6] >> (i & 63)) & 1ull;
  return bad ? (uint64_t)G.ph_len : G.offsets[i + 1] - G.offsets[i];
}
__device__ __forceinline__ uint64_t wave_incl_scan64(uint64_t v, uint32_t lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t up = __shfl_up(v, d, 64);
    if ((int)lane >= d) v += up;
  }
  return v;
}
// inclusive scan over the kPatchBlock threads of a workgroup; *total = the workgroup's sum.  Contains two barriers.
__device__ __forceinline__ uint64_t block_incl_scan64(uint64_t v, uint64_t* wt, uint64_t* total) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t incl = wave_incl_scan64(v, lane);
  __syncthreads();                       // (wt may still be read from the previous round)
  if (lane == 63) wt[wave] = incl;
  __syncthreads();
  uint64_t base = 0;
  for (uint32_t w = 0; w < wave; w++) base += wt[w];
  *total = wt[0] + wt[1] + wt[2] + wt[3];
  return base + incl;
}

extern "C" __global__ void __launch_bounds__(kPatchBlock) rh_k_patch_lens(GParams G) {
  __shared__ uint64_t wt[4];
  uint64_t total;
  block_incl_scan64(patched_len(G, (uint64_t)blockIdx.x * kPatchBlock + threadIdx.x), wt, &total);
  if (threadIdx.x == 0) G.blocksum[blockIdx.x] = total;
}

// one workgroup: blocksum[] -> its exclusive prefix, in place
extern "C" __global__ void __launch_bounds__(kPatchBlock) rh_k_patch_scan(GParams G) {
  __shared__ uint64_t wt[4];
  uint64_t carry = 0;
  for (uint32_t base = 0; base < G.nblocks; base += kPatchBlock) {
    const uint32_t i = base + threadIdx.x;
    const uint64_t v = i < G.nblocks ? G.blocksum[i] : 0;
    uint64_t total;
    const uint64_t incl = block_incl_scan64(v, wt, &total);
    if (i < G.nblocks) G.blocksum[i] = carry + incl - v;
    carry += total;
  }
}

extern "C" __global__ void __launch_bounds__(kPatchBlock) rh_k_patch_offsets(GParams G) {
  __shared__ uint64_t wt[4];
  const uint64_t i = (uint64_t)blockIdx.x * kPatchBlock + threadIdx.x;
  const uint64_t v = patched_len(G, i);
  uint64_t total;
  const uint64_t incl = block_incl_scan64(v, wt, &total);
  const uint64_t base = G.blocksum[blockIdx.x];
  if (i < G.n) G.new_offsets[i] = base + incl - v;
  if (i + 1 == G.n) G.new_offsets[G.n] = base + incl;
}

// --------------------------------------------------------------------------
// patch: gather
// --------------------------------------------------------------------------
// `len` bytes from s to d by one wavefront.  d and s are misaligned against each other in general: the vectors are cut where the
// DESTINATION is 16-byte aligned (aligned stores, unaligned loads), the bytes in front of the first and behind the last one go singly.
__device__ __forceinline__ void wave_copy(uint8_t* d, const uint8_t* s, uint64_t len, uint32_t lane) {
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

extern "C" __global__ void __launch_bounds__(kBlock) rh_k_patch_gather(GParams G) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t w = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);      // this wavefront's bitmap word
  const uint64_t r0 = w << 6;
  if (r0 >= G.n) return;
  const uint32_t cnt = G.n - r0 < 64 ? (uint32_t)(G.n - r0) : 64u;
  const uint64_t bad = G.bitmap[w] & (cnt == 64 ? ~0ull : ((1ull << cnt) - 1ull));
  uint32_t j = 0;
  while (j < cnt) {                                                // (everything here is wave-uniform)
    if ((bad >> j) & 1ull) {
      uint8_t* d = G.out + G.new_offsets[r0 + j];
      for (uint32_t b = lane; b < G.ph_len; b += 64) d[b] = G.ph[b];
      j++;
      continue;
    }
    const uint64_t rest = bad >> j;
    const uint32_t e = rest ? j + (uint32_t)__builtin_ctzll(rest) : cnt;      // records [j, e) are well-formed neighbours
    const uint64_t s0 = G.offsets[r0 + j], s1 = G.offsets[r0 + e];
    wave_copy(G.out + G.new_offsets[r0 + j], G.data + s0, s1 - s0, lane);
    j = e;
  }
}

}  // namespace rh

// --------------------------------------------------------------------------
// launchers (engine_tolerant.cpp)
// --------------------------------------------------------------------------
extern "C" uint32_t rh_validate_lds_fixed(int list_depth) { return (uint32_t)(list_depth > 0 ? list_depth : 1) * rh::kBlock * 4; }

extern "C" int rh_launch_validate(const rh::VParams* V, uint32_t lds_bytes, void* stream) {
  (void)hipGetLastError();
  int e = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(rh::rh_k_validate), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (e) return e;
  const uint32_t nblocks = (uint32_t)((V->n + rh::kBlock - 1) / rh::kBlock);
  hipLaunchKernelGGL(rh::rh_k_validate, dim3(nblocks), dim3(rh::kBlock), lds_bytes, (hipStream_t)stream, *V);
  return (int)hipGetLastError();
}

// lengths, scan, offsets: new_offsets[0..n] are complete in stream order behind this
extern "C" int rh_launch_patch_offsets(const rh::GParams* G, void* stream) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(rh::rh_k_patch_lens, dim3(G->nblocks), dim3(rh::kPatchBlock), 0, (hipStream_t)stream, *G);
  hipLaunchKernelGGL(rh::rh_k_patch_scan, dim3(1), dim3(rh::kPatchBlock), 0, (hipStream_t)stream, *G);
  hipLaunchKernelGGL(rh::rh_k_patch_offsets, dim3(G->nblocks), dim3(rh::kPatchBlock), 0, (hipStream_t)stream, *G);
  return (int)hipGetLastError();
}

extern "C" int rh_launch_patch_gather(const rh::GParams* G, void* stream) {
  (void)hipGetLastError();
  const uint64_t waves = (G->n + 63) / 64;
  hipLaunchKernelGGL(rh::rh_k_patch_gather, dim3((uint32_t)((waves + 3) / 4)), dim3(rh::kBlock), 0, (hipStream_t)stream, *G);
  return (int)hipGetLastError();
}
