// CDNA4 (gfx950) kernel of the container read (rh_decode_blocks).
//
//   rh_k_split   "blocks" -> "record offsets".  An Avro container block says "N records, M bytes" and nothing says where record
//                j starts: the only way to find out is to walk records 0 .. j - 1 with the writer's schema.  One lane per block
//                runs the generic interpreter's CAREFUL walk with nothing stored and nothing counted (the walk of rh_k_validate:
//                every op the way walk_drop.h runs the ops of a dropped field) once per record of its block, from global
//                memory, and notes where every record began.  The program counter is wave-uniform; a lane whose block has
//                fewer records than its neighbours' sits the other iterations out.
//   rh_k_split_where   the same kernel with a predicate evaluated in the walk: a keep bit per record beside the
//                offsets, for the filtered container reads (rh_decode_blocks_where, rh_filter_blocks).
// The walk reads every byte once, one dependent stream per lane, and a wavefront takes as long as its fullest block: the
// parallelism is the number of blocks ("What bounds it").
#include <hip/hip_runtime.h>
#include <stdint.h>

#define RH_DEEP 1      // as the interpreter of kernels.hip: any nesting the schema front-end accepts

#include "kernel_common.h"
#include "program.h"
#include "walk.h"
#include "walk_drop.h"
#include "container.h"
#include "filter_eval.h"             // filter_walk: the split walk that also evaluates a predicate (shared with filter.hip)
#include "container_where_core.h"    // the keep-word accumulation of rh_k_split_where

namespace rh {

// what DropCtx needs of the walk's context (validate.hip VCtx): list framing and the enum symbols
struct SCtx {
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

typedef const __attribute__((address_space(4))) Op* SProgPtr;
__device__ __forceinline__ Op s_ld_op(SProgPtr p) {
  Op o;
  o.code = p->code; o.flags = p->flags; o.dom = p->dom; o.a = p->a; o.b = p->b; o.c = p->c;
  o.buf0 = p->buf0; o.buf1 = p->buf1; o.buf2 = p->buf2; o.node = p->node;
  return o;
}

// one record per live lane: the program, every op counters-only and careful (validate.hip validate_walk)
template <class Src>
__device__ __forceinline__ void split_walk(const Op* program, const SCtx& c, const Src& src, Lane& L) {
  const SProgPtr prog = reinterpret_cast<SProgPtr>(reinterpret_cast<uintptr_t>(program));
  int pc = 0;
  for (;;) {
    pc = __builtin_amdgcn_readfirstlane(pc);
    const Op op = s_ld_op(prog + pc);
    if (op.code == OP_END) return;
    int npc = op.code == OP_LIST_TAIL ? op.b : pc + 1;      // LIST_TAIL goes back to its LIST_NEXT
    if (op.code > OP_BIN) return;
    if (!run_dropped<false, true>(c, src, L, op)) npc = op.b;      // no lane has an item left: to LIST_END
    pc = npc;
  }
}

// The body of rh_k_split and of rh_k_split_salvage.  SALVAGE: the lane leaves rec[b] for its block whatever became of it, and
// S.err is not written; everything else -- the walk, the offsets, the order of the stores -- is the same code.
template <bool SALVAGE>
__device__ __forceinline__ void split_body(const SParams& S, SalvageRec* rec) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t depth = (uint32_t)(S.list_depth > 0 ? S.list_depth : 1);
  uint32_t* const rem = reinterpret_cast<uint32_t*>(smem);
  for (uint32_t d = 0; d < depth; d++) rem[d * kBlock + tid] = 0;
  __syncthreads();

  const uint64_t b = (uint64_t)blockIdx.x * kBlock + tid;
  const bool mine = b < (uint64_t)S.nb;
  uint64_t st = 0, en = 0, f0 = 0, f1 = 0;
  if (mine) { st = S.start[b]; en = S.end[b]; f0 = S.first[b]; f1 = S.first[b + 1]; }
  const uint64_t cnt = f1 - f0;
  // the lane's source is based at its own block: cursors stay 32-bit (the host refuses a block of 4 GiB - 16 or more)
  const uint64_t base = st & ~15ull;
  const GlobalSrc src{S.data + base, S.data_len - base};
  const uint32_t cur0 = (uint32_t)(st - base), end = cur0 + (uint32_t)(en - st);

  SCtx c;
  c.rem = rem; c.sym_off = S.sym_off; c.sym_data = S.sym_data;
  c.lrow = tid; c.tid = tid; c.lane = lane; c.wave_live = true;
  Lane L;
  L.cur = cur0; L.end = end; L.err = 0; L.edetail = 0;
  uint32_t code = 0;
  int64_t detail = 0;
  unsigned long long key = 0;
  uint64_t j = 0;
  uint32_t bad_at = 0;      // SALVAGE: where the malformed record began
  for (;;) {
    const bool go = mine && code == 0 && j < cnt;
    if (!__any(go)) break;      // (wave-uniform)
    const uint32_t at = L.cur;
    if (go) S.offsets[f0 + j] = st + (uint64_t)(at - cur0);
    L.err = 0; L.edetail = 0;
    L.live = go; L.pres = go; L.redo = false; L.la = 0;
    L.pstk = 0; L.lstk = 0; L.sstk = 0;
    split_walk(S.prog, c, src, L);
    if (go && L.err) { code = L.err; detail = L.edetail; key = split_key_record(f0 + j); bad_at = at; }
    if (!go) L.cur = at;        // (a lane that sat the record out stays where it was)
    j += go ? 1u : 0u;
  }
  if (mine && code == 0 && L.cur != end) { code = E_BLOCK_END; detail = (int64_t)(L.cur - cur0); key = split_key_block(f1); }
  if (mine && code != 0) {
    if constexpr (!SALVAGE) {
      SplitErr e; e.code = code; e.pad = 0; e.detail = detail;
      S.err[b] = e;
    }
    atomicMax(S.first_bad, ~key);
  }
  if constexpr (SALVAGE) {
    if (mine) {
      // j counts the records walked, the malformed one among them; L.cur of a lane that failed is not where a record ends
      const bool rec_bad = code != 0 && code != E_BLOCK_END;
      SalvageRec r;
      r.code = code; r.pad = 0; r.detail = detail;
      r.kept = rec_bad ? j - 1 : j;
      r.kept_end = st + (uint64_t)((rec_bad ? bad_at : L.cur) - cur0);
      rec[b] = r;
    }
  }
  if (mine && b + 1 == (uint64_t)S.nb) S.offsets[f1] = en;      // offsets[n]: the last record ends with the last block
}

extern "C" __global__ void __launch_bounds__(kBlock) rh_k_split(SParams S) { split_body<false>(S, nullptr); }

// rh_k_split_salvage: the same walk; a lane that fails stops ITS block and says how far it came.
extern "C" __global__ void __launch_bounds__(kBlock) rh_k_split_salvage(SalvageParams P) { split_body<true>(P.S, P.rec); }

// rh_k_split_where: rh_k_split -- the geometry, the block-based source, the offsets, the verdicts, all as
// split_body<false> has them -- with filter_eval.h's filter_walk in place of split_walk: the one careful walk of every record
// also says whether the record matches.  The lanes of a wavefront are at unrelated record indices, so there is no ballot: a lane
// gathers the bits of one keep word in a register (container_where_core.h) and ORs it into W.keep -- zero at launch -- when it
// moves on to the next word and when its block ends.  Nothing in this launch reads W.keep: the next launch does, so no fence.
// A lane that sits an iteration out (go == false) runs the walk with L.live = false and f_eval's reads at its resting cursor:
// at <= end <= S.data_len - base, and GlobalSrc bounds every read by that; its verdict is dropped (`go && ...`).  A lane that
// fails stops its block: the records behind the malformed one have no bit and no offset, and the call fails on the host.
extern "C" __global__ void __launch_bounds__(kBlock) rh_k_split_where(SWParams W) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  __shared__ unsigned long long wg_kept;
  const SParams& S = W.S;
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t depth = (uint32_t)(S.list_depth > 0 ? S.list_depth : 1);
  uint32_t* const rem = reinterpret_cast<uint32_t*>(smem);
  for (uint32_t d = 0; d < depth; d++) rem[d * kBlock + tid] = 0;
  if (tid == 0) wg_kept = 0;
  __syncthreads();

  const uint64_t b = (uint64_t)blockIdx.x * kBlock + tid;
  const bool mine = b < (uint64_t)S.nb;
  uint64_t st = 0, en = 0, f0 = 0, f1 = 0;
  if (mine) { st = S.start[b]; en = S.end[b]; f0 = S.first[b]; f1 = S.first[b + 1]; }
  const uint64_t cnt = f1 - f0;
  const uint64_t base = st & ~15ull;      // (as rh_k_split: the source is based at the block, cursors stay 32-bit)
  const GlobalSrc src{S.data + base, S.data_len - base};
  const uint32_t cur0 = (uint32_t)(st - base), end = cur0 + (uint32_t)(en - st);

  SCtx c;
  c.rem = rem; c.sym_off = S.sym_off; c.sym_data = S.sym_data;
  c.lrow = tid; c.tid = tid; c.lane = lane; c.wave_live = true;
  Lane L;
  L.cur = cur0; L.end = end; L.err = 0; L.edetail = 0;
  uint32_t code = 0;
  int64_t detail = 0;
  unsigned long long key = 0;
  uint64_t j = 0, nkept = 0;
  KeepAcc acc;
  keep_acc_init(acc, f0);
  const FMarks marks = f_marks(*W.flt);
  for (;;) {
    const bool go = mine && code == 0 && j < cnt;
    if (!__any(go)) break;      // (wave-uniform)
    const uint32_t at = L.cur;
    if (go) S.offsets[f0 + j] = st + (uint64_t)(at - cur0);
    L.err = 0; L.edetail = 0;
    L.live = go; L.pres = go; L.redo = false; L.la = 0;
    L.pstk = 0; L.lstk = 0; L.sstk = 0;
    const bool match = filter_walk(S.prog, W.flt, marks, W.cbytes, c, src, L, go);
    if (go && L.err) { code = L.err; detail = L.edetail; key = split_key_record(f0 + j); }
    if (go && code == 0) {      // (f0 + j < f1 <= n: the word is inside W.keep)
      uint64_t fw = 0, fb = 0;
      if (keep_acc_step(acc, f0 + j, match, &fw, &fb)) atomicOr(reinterpret_cast<unsigned long long*>(W.keep + fw), (unsigned long long)fb);
      nkept += match ? 1u : 0u;
    }
    if (!go) L.cur = at;        // (a lane that sat the record out stays where it was)
    j += go ? 1u : 0u;
  }
  if (mine && keep_acc_finish(acc)) atomicOr(reinterpret_cast<unsigned long long*>(W.keep + acc.word), (unsigned long long)acc.bits);
  if (mine && code == 0 && L.cur != end) { code = E_BLOCK_END; detail = (int64_t)(L.cur - cur0); key = split_key_block(f1); }
  if (mine && code != 0) {
    SplitErr e; e.code = code; e.pad = 0; e.detail = detail;
    S.err[b] = e;
    atomicMax(S.first_bad, ~key);
  }
  if (mine && b + 1 == (uint64_t)S.nb) S.offsets[f1] = en;      // offsets[n]: the last record ends with the last block

  // the kept count: per wavefront, per workgroup in LDS, one add into slot (workgroup & 63) as rh_k_filter
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) nkept += __shfl_down(nkept, d, 64);
  if (lane == 0 && nkept) atomicAdd(&wg_kept, (unsigned long long)nkept);
  __syncthreads();
  if (tid == 0 && wg_kept) atomicAdd(W.kept + (blockIdx.x & (kFilterSlots - 1)), wg_kept);
}

// rh_k_salvage_gather: what the salvage keeps, made contiguous.  One wavefront per keeping block copies the block's kept run to
// its 16-byte aligned place (aligned 16-byte stores, loads at whatever alignment the source has, the tail byte by byte), zeroes
// the pad behind it and rebases the run's record offsets.  Every branch below is wave-uniform but the lane-strided loops and
// the single-lane stores, and no step is cooperative: a lane that leaves a loop early waits for nobody.
// Bounds (the host's, engine_container.cpp salvage_and_decode): src + len = kept_end <= the block's end <= the buffer; dst + len <=
// dst_next <= out_len; new_first + kept <= n'.
extern "C" __global__ void __launch_bounds__(kBlock) rh_k_salvage_gather(SalvageGatherParams G) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t w = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (w >= (uint64_t)G.njobs) return;
  const GatherJob J = G.jobs[w];
  if (J.dst_next > G.out_len || J.len > J.dst_next - J.dst) return;      // (never: the host laid the runs out)
  const uint8_t* const s = G.data + J.src;
  uint8_t* const d = G.out + J.dst;
  const uint64_t nvec = J.len >> 4;
  for (uint64_t v = lane; v < nvec; v += 64) {
    const v4w x = *reinterpret_cast<const v4wu*>(s + (v << 4));
    *reinterpret_cast<v4w*>(d + (v << 4)) = x;
  }
  const uint64_t done = nvec << 4;
  if (done + lane < J.len) d[done + lane] = s[done + lane];          // (fewer than 16 bytes are left)
  const uint64_t room = J.dst_next - J.dst;
  if (J.len + lane < room) d[J.len + lane] = 0;                      // (the pad: fewer than 16 bytes)
  const uint64_t* const off = G.off + J.off_first;
  uint64_t* const noff = G.new_off + J.new_first;
  for (uint64_t j = lane; j < J.kept; j += 64) noff[j] = off[j] - J.src + J.dst;
  if (J.last && lane == 0) noff[J.kept] = J.dst + J.len;
}

}  // namespace rh

// --------------------------------------------------------------------------
// launcher (engine_container.cpp)
// --------------------------------------------------------------------------
extern "C" uint32_t rh_split_lds_bytes(int list_depth) { return (uint32_t)(list_depth > 0 ? list_depth : 1) * rh::kBlock * 4; }

extern "C" int rh_launch_split(const rh::SParams* S, void* stream) {
  (void)hipGetLastError();
  if (S->nb == 0) return 0;
  const uint32_t lds = rh_split_lds_bytes(S->list_depth);
  int e = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(rh::rh_k_split), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (e) return e;
  const uint32_t nblocks = (S->nb + rh::kBlock - 1) / rh::kBlock;
  hipLaunchKernelGGL(rh::rh_k_split, dim3(nblocks), dim3(rh::kBlock), lds, (hipStream_t)stream, *S);
  return (int)hipGetLastError();
}

// W->keep and W->kept are zero in stream order in front of this (the caller's memset)
extern "C" int rh_launch_split_where(const rh::SWParams* W, void* stream) {
  (void)hipGetLastError();
  if (W->S.nb == 0) return 0;
  const uint32_t lds = rh_split_lds_bytes(W->S.list_depth);
  int e = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(rh::rh_k_split_where), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 64);
  if (e) return e;
  const uint32_t nblocks = (W->S.nb + rh::kBlock - 1) / rh::kBlock;
  hipLaunchKernelGGL(rh::rh_k_split_where, dim3(nblocks), dim3(rh::kBlock), lds, (hipStream_t)stream, *W);
  return (int)hipGetLastError();
}

extern "C" int rh_launch_split_salvage(const rh::SalvageParams* P, void* stream) {
  (void)hipGetLastError();
  if (P->S.nb == 0) return 0;
  const uint32_t lds = rh_split_lds_bytes(P->S.list_depth);
  int e = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(rh::rh_k_split_salvage), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (e) return e;
  const uint32_t nblocks = (P->S.nb + rh::kBlock - 1) / rh::kBlock;
  hipLaunchKernelGGL(rh::rh_k_split_salvage, dim3(nblocks), dim3(rh::kBlock), lds, (hipStream_t)stream, *P);
  return (int)hipGetLastError();
}

extern "C" int rh_launch_salvage_gather(const rh::SalvageGatherParams* G, void* stream) {
  (void)hipGetLastError();
  if (G->njobs == 0) return 0;
  const uint32_t waves_per_group = rh::kBlock / 64;
  hipLaunchKernelGGL(rh::rh_k_salvage_gather, dim3((G->njobs + waves_per_group - 1) / waves_per_group), dim3(rh::kBlock), 0, (hipStream_t)stream, *G);
  return (int)hipGetLastError();
}
