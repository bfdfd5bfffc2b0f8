// Column projection (rh_schema_project): ops of top-level fields the caller did not ask for.
//
// A projected schema program keeps the op sequence of the full schema -- wire order is field order, every field has to be
// walked to find the next one -- but the ops of a dropped field carry F_DROP: no buffers, no node, no counter, no child row
// domain.  Such an op is run by the EXISTING handler of walk.h in its counters-only form (EMIT = false) over a view of the
// walk's context whose counter() lands in a dead register (the pattern of walk.h SkipCtx): validation, cursor movement and
// list framing are the code every un-projected walk runs, nothing is stored and nothing is counted.
//   size walk:           <EMIT = false, CAREFUL> as for every other op, counters discarded
//   emit walk, trusted:  <EMIT = false, fast>, every anomaly predicate dropped (kSkip: the size pass cleared the tile)
//   emit walk, careful:  <EMIT = false, careful>, the size walk's checks and error order
// Included by the generated source of projected schemas (specialize.cpp) and by the generic interpreter (kernels.hip); the
// flag lives here and not in program.h so that the kernels of un-projected schemas -- generated source and the headers it
// includes -- stay byte for byte what they were (the kernel-cache key hashes them, rtc_compile.cpp).
#pragma once
#include "program.h"

namespace rh {

constexpr int32_t F_DROP = 32;   // OpFlags: the op belongs to a dropped top-level field (buf0 = buf1 = node = -1; `a` names no counter)

}  // namespace rh

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
#include "walk.h"

namespace rh {

// TRUSTED: the bytes were cleared by the size pass of this call (the emit walk's fast form) -- walk.h RH_TRUST
template <class C, bool TRUSTED>
struct DropCtx {
  static constexpr bool kSkip = TRUSTED;
  static constexpr bool kWide = C::kWide;
  static constexpr bool kEnumImm = C::kEnumImm;
  static constexpr bool kWaveCtr = false;             // (nothing is counted: neither per lane nor per wavefront)
  __device__ __forceinline__ void wave_total(int, uint32_t) const {}
  __device__ __forceinline__ uint32_t wave_offset(int, uint32_t) const { return 0; }
  static __device__ __forceinline__ bool enum_sym(int b, uint32_t v, uint32_t& len, uint64_t& bits) { return C::enum_sym(b, v, len, bits); }
  const C& base;
  const uint32_t* sym_off;
  const uint8_t* sym_data;
  uint32_t lrow, lane;
  bool wave_live;
  mutable uint32_t dead = 0;                          // every counter of a dropped field
  __device__ __forceinline__ explicit DropCtx(const C& b)
      : base(b), sym_off(b.sym_off), sym_data(b.sym_data), lrow(b.lrow), lane(b.lane), wave_live(b.wave_live) {}
  __device__ __forceinline__ uint32_t& counter(int) const { return dead; }
  __device__ __forceinline__ uint32_t& remaining(int d) const { return base.remaining(d); }      // (list framing is real: the block loop runs)
  // (the EMIT side of the handlers is dead code under EMIT = false, but it has to compile)
  __device__ __forceinline__ void* buf(int) const { return nullptr; }
  __device__ __forceinline__ uint32_t gbase(int) const { return 0; }
  template <bool ACC> __device__ __forceinline__ void add_nulls_wave(int, uint32_t) const {}
  __device__ __forceinline__ void add_nulls_lane(int) const {}
  template <bool ACC> __device__ __forceinline__ void put_word0(int, uint64_t) const {}
  __device__ __forceinline__ void set_bit(int, int, uint32_t) const {}
};

// One dropped op with a run-time Op (the generic interpreter).  False: a LIST_NEXT that found no lane with an item left.
template <bool EMIT, bool CAREFUL, class Ctx, class Src>
__device__ __forceinline__ bool run_dropped(const Ctx& c, const Src& src, Lane& L, const Op& op) {
  const DropCtx<Ctx, (EMIT && !CAREFUL)> dc(c);
  switch (op.code) {
    case OP_FIXED: h_fixed<false, CAREFUL>(dc, src, L, op); break;
    case OP_STRING:
    case OP_ENUM: h_string<false, CAREFUL>(dc, src, L, op); break;
    case OP_BIN: h_bin<false, CAREFUL>(dc, src, L, op); break;
    case OP_REC_BEGIN: h_rec_begin<false, CAREFUL>(dc, src, L, op); break;
    case OP_REC_END: h_rec_end(L); break;
    case OP_UNION_BEGIN: h_union_begin<false, CAREFUL>(dc, src, L, op); break;
    case OP_VARIANT: h_variant(L, op); break;
    case OP_UNION_END: h_union_end(L); break;
    case OP_LIST_BEGIN: h_list_begin<false, CAREFUL>(dc, src, L, op); break;
    case OP_LIST_NEXT: return h_list_next<CAREFUL, (EMIT && !CAREFUL)>(dc, src, L, op);
    case OP_LIST_TAIL: h_list_tail(dc, L, op); break;
    case OP_LIST_END: h_list_end<false>(dc, L, op); break;
    default: break;
  }
  return true;
}

}  // namespace rh
#endif
