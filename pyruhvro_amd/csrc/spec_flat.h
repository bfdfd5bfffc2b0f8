// Emit kernels of a schema whose calls have NO SIZE PASS: no variable-length output (K == 0), and not a projection that keeps the
// pass for the fields it dropped (schema.h size_always).  Included only by the generated source of such schemas (specialize.cpp),
// and only then part of the kernel-cache key (rtc_compile.cpp): spec_body.h and the kernels of every other schema are byte for
// byte what they were.
//
// Without a size pass nobody classifies a call's tiles: none is refused for want of the ranged pair (LF_NEED_RANGED), listed
// or counted.  spec_emit<S, false> returns on a tile past the LDS window -- it is the pair's -- so in a call that did not launch the
// pair (AUTO kernels, a schema whose history knows no such tile: eight long columns of small values have a mean record of ~10 bytes
// and an 8 KiB window; 256 records of 10-byte varints are 20 KB) the rows of that tile kept what the pooled arena held, and the call
// returned success.  Here
//   * rh_spec_emit walks such a tile itself when P.ranged == 0: the careful walk straight from global memory (spec_run_walk, the
//     arm the single-pass kernel uses) -- one dependent HBM round trip per head, but no extra pass and no repeat of the call;
//   * every tile past the window is counted into the call's tile statistics (control words 9 and, walked in ranges by
//     rh_spec_emit_r, 11: kernels.hip tile_stats_commit's order), which leave with the head of the control block: the host's
//     counters advance and the schema's next calls launch the ranged pair (engine_device_call.cpp learn_unsized_tiles).
// Tiles that fit take spec_emit as it is.
#pragma once
#include "spec_body.h"

namespace rh {

constexpr int kStatOverWindowWord = 9, kStatSubtiledWord = 11;      // words of the control block (u32 index): the tile statistics

template <class S, bool RANGED = false>
__device__ __forceinline__ void spec_emit_flat(const KParams& P) {
  static_assert(S::K == 0 && S::KL == 0 && S::NBM == 0, "spec_emit_flat: schemas without counters only");
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  if (reinterpret_cast<const uint32_t*>(P.first_bad)[2] != 0) return;      // the layout kernel refused: nothing to emit (final before this kernel starts)
  constexpr int T = TileOf<S>::T, NW = TileOf<S>::NW;
  const uint32_t tid = threadIdx.x;
  uint32_t tile = 0;
  if constexpr (RANGED) { if (!ranged_tile_of_block(P, blockIdx.x, tile)) return; }
  else tile = tile_of_block(blockIdx.x, P.nblocks);
  const Geo g = geometry<T>(P, tile);
  const uint64_t wb = P.offsets[g.rec0], we = P.offsets[g.rec0 + g.nrec];
  const uint64_t wb16 = wb & ~15ull;
  const bool fits = (we - wb16) <= (uint64_t)P.win_bytes;      // (workgroup-uniform, like everything above: ahead of every barrier)
  if (fits) {
    if constexpr (!RANGED) spec_emit<S, false>(P);
    return;
  }
  if constexpr (RANGED) {
    if (tid == 0) {
      atomicAdd(reinterpret_cast<uint32_t*>(P.first_bad) + kStatOverWindowWord, 1u);
      atomicAdd(reinterpret_cast<uint32_t*>(P.first_bad) + kStatSubtiledWord, 1u);
    }
    spec_emit<S, true>(P);
    return;
  } else {
    if (P.ranged != 0) return;                                  // rh_spec_emit_r follows in this call: its tile
    if (tid == 0) atomicAdd(reinterpret_cast<uint32_t*>(P.first_bad) + kStatOverWindowWord, 1u);
    // spec_emit for a tile that is not staged: no counters to load or scan (K == 0), every record walked carefully from global memory
    const SpecSmem<S> s(P, smem);
    uint64_t o0 = 0, o1 = 0;
    if (tid < g.nrec) { o0 = P.offsets[g.rec0 + tid]; o1 = P.offsets[g.rec0 + tid + 1]; }
    Lane L;
    SCtx<S> c;
    spec_ctx_init(c, P, s, g, tid);
    c.bufp = (const __attribute__((address_space(4))) uint64_t*)(reinterpret_cast<uintptr_t>(P.bufptr) + (size_t)g.chunk * S::NBUF * 8);
    for (int i = tid; i < S::NNODES; i += T) s.nullcnt[i] = 0;
    for (int i = tid; i < S::NNODES * NW; i += T) s.nullw[i] = 0;
    if (tid == 0) s.misc[0] = 0xFFFFFFFFu;
    __syncthreads();
    lane_init_from(L, g, o0, o1, wb16, tid);
    spec_run_walk<S, true, true>(P, c, s.win, L, false, wb16);
    report_errors(P, s.misc, L, g, tid, tile);   // barrier inside: nullcnt complete
    for (int i = tid; i < S::NNODES; i += T) {
      uint32_t v = s.nullcnt[i];
      for (int w = 0; w < NW; w++) v += s.nullw[i * NW + w];
      if (v) atomicAdd(&P.nullcount[((size_t)i * P.k + g.chunk) * P.null_slots + (tile & (P.null_slots - 1))], v);
    }
    if constexpr (S::NB0 > 0) {   // the tile's domain-0 bitmap words (SCtx::put_word0): one lane per word
      for (uint32_t i = tid; i < (uint32_t)(S::NB0 * NW); i += T) {
        const uint32_t slot = i / NW, w = i % NW;
        if (w * 64u < g.nrec) st_global<uint64_t, false>(c.buf(S::bm0buf(slot)), (g.lrow0 >> 6) + w, c.bmw0[i]);
      }
    }
  }
}

}  // namespace rh
