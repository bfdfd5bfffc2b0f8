// Reader schemas (rh_schema_resolve): the two kinds of op a resolved schema program has beyond a projected one's.
//
// A resolved program walks the WRITER's wire form and builds the READER's columns (schema.cpp compile_schema_resolved).
// Writer fields the reader lacks are F_DROP ops (walk_drop.h); this header adds
//   * promoted leaves: an OP_FIXED whose `a` is the kind on the WIRE (int / long / float) and whose flags carry the kind
//     that is STORED (long / float / double) -- h_fixed_p: h_fixed's wire side (the same read_head forms, head fusion, fast /
//     careful / trusted variants), a conversion, and the store of the reader's width.  Validity and null counts are h_fixed's.
//   * defaulted leaves (F_CONST): a reader field the writer lacks.  The host encodes the default once as the Avro datum of
//     the reader field's type (union branch index, then the value) into the symbol blob that travels with the program
//     (sym_data; op.b = position, op.c = bytes, 16 zero bytes behind it).  The op runs through the EXISTING handler over a
//     ConstSrc -- a source that reads that blob, at a wave-uniform address -- with the record's cursor set aside: the size
//     walk counts a default string's bytes like any other string's, so scan, layout, null counts and lazy bitmaps need no
//     code of their own.  Only leaf defaults exist, so no list framing ever runs over a ConstSrc.
// string <-> bytes changes the Arrow type only and needs nothing here.
// Included by the generated source of resolved schemas (specialize.cpp) and by the generic interpreter's projected entries
// (kernels.hip); the flags live here, like F_DROP, so that every other kernel stays byte for byte what it was.
#pragma once
#include "walk_drop.h"

namespace rh {

constexpr int32_t F_CONST = 64;            // OpFlags: OP_FIXED / OP_STRING of a defaulted reader field (b = blob position in sym_data, c = bytes)
constexpr int32_t kPromoteShift = 7;       // OpFlags bits 7..9: 0 = not promoted, else 1 + the FixedKind that is stored
constexpr int32_t F_PROMOTE_MASK = 7 << kPromoteShift;
constexpr int32_t F_RESOLVE_MASK = F_CONST | F_PROMOTE_MASK;
constexpr uint32_t kConstSlack = 16;       // zero bytes behind every default in the blob
constexpr uint32_t kMaxDefaultBytes = 255; // a string / bytes default is at most this long (below walk.h kCoopMin: every lane copies its own)
RH_HD inline int32_t promote_flags(int32_t stored_kind) { return (stored_kind + 1) << kPromoteShift; }
RH_HD inline int32_t stored_kind(int32_t flags) { return ((flags & F_PROMOTE_MASK) >> kPromoteShift) - 1; }

}  // namespace rh

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)

namespace rh {

// int / long / float leaf read as the writer wrote it, stored as the reader declares it (Avro 1.11 "Schema Resolution":
// int -> long, float, double; long -> float, double; float -> double).  Integer to float is the C cast: ONE rounding, to
// nearest even (a long goes to float directly, never through a double).
template <bool EMIT, bool CAREFUL, int LA = 0, class Src, class Ctx>
__device__ __forceinline__ void h_fixed_p(const Ctx& c, const Src& src, Lane& L, const Op& op) {
  const int32_t rk = stored_kind(op.flags);
  const bool act = L.live;
  const bool dec = act && L.pres;
  const bool is_int = op.a != FK_F32;
  int64_t v = 0;
  void* const pf1 = EMIT ? c.buf(op.buf1) : nullptr;     // requested ahead of the head: see h_string
  const bool isval = read_head<CAREFUL, RH_TRUST, (CAREFUL ? 0 : LA)>(src, L, dec, (op.flags & F_NULLABLE) != 0, (op.flags & F_NULL_FIRST) != 0, is_int,
                                        op.a == FK_I64, v);
  uint64_t bits;
  bool valid;
  if (is_int) {
    valid = isval && L.live;
    if (rk == FK_I64) {
      bits = (uint64_t)v;                                 // (read_head sign-extends an int)
    } else if (rk == FK_F32) {
      const float f = op.a == FK_I32 ? (float)(int32_t)v : (float)v;
      bits = (uint64_t)__float_as_uint(f);
    } else {
      const double d = op.a == FK_I32 ? (double)(int32_t)v : (double)v;
      bits = (uint64_t)__double_as_longlong(d);
    }
  } else {
    // (head fusion, read_head: a float without a null union may open or continue a chain)
    constexpr int la = CAREFUL ? 0 : LA;
    uint64_t x;
    if constexpr ((la & 1) != 0) x = L.la;
    else if constexpr ((la & 2) != 0 && (la >> 2) == 8) x = src.ld8(L.cur);
    else if constexpr ((la & 2) != 0) x = (uint64_t)src.ld4(L.cur);
    else x = src.ld5(L.cur);
    const uint32_t avail = L.end - L.cur;
    const bool want = isval && L.live;
    const bool eob = (!CAREFUL && !RH_TRUST) ? false : (want && avail < 4u);      // (fast size walk: see read_head)
    RH_REJECT_SOFT(L, eob, E_EOB_F32);
    valid = want && L.live;
    L.cur += valid ? 4u : 0u;
    if constexpr ((la & 2) != 0) L.la = x >> (8u * (valid ? 4u : 0u));
    bits = (uint64_t)__double_as_longlong((double)__uint_as_float((uint32_t)x));   // exact; subnormals and NaN payloads kept
  }
  if (!valid) bits = 0;   // zero under nulls (arrow-rs append_null)
  uint32_t row = 0;
  if (EMIT) {
    row = row_of(c, op.dom);
    if (act) {
      if (rk == FK_F32) st_global<uint32_t, Ctx::kWide>(pf1, row, (uint32_t)bits);
      else st_global<uint64_t, Ctx::kWide>(pf1, row, bits);
    }
  }
  put_validity<EMIT, Src::kSlide>(c, op, act, valid, row);
}

// The default blob as a source: GlobalSrc's bounded reads at positions every lane shares.  kSlide is the enclosing walk's
// (a ranged walk accumulates its bitmap words and null counts, walk.h put_validity ACC); `lanes`: a string is copied by its
// own lane, never by the wavefront together.
template <bool SLIDE>
struct ConstSrc : GlobalSrc {
  static constexpr bool kSlide = SLIDE;
  static constexpr bool kMoves = false;
  static constexpr bool sliding = false;
  static constexpr bool lanes = true;
  __device__ __forceinline__ ConstSrc(const uint8_t* blob, uint64_t readable) { g = blob; lim = readable; }
  template <class LaneT>
  __device__ __forceinline__ void refill(LaneT&, uint32_t) const {}
  __device__ __forceinline__ uint32_t advance_to(uint32_t, uint32_t, int) const { return 0; }
  __device__ __forceinline__ void sync(int) const {}
};

// One defaulted leaf: the op's ordinary handler over the blob, the record's cursor set aside.  The blob is the engine's own
// encoding, so no lane can fail or leave the fast wire forms here.
template <bool EMIT, bool CAREFUL, class Ctx, class Src>
__device__ __forceinline__ void run_const(const Ctx& c, const Src&, Lane& L, const Op& op) {
  const ConstSrc<Src::kSlide> ks(c.sym_data, (uint64_t)(uint32_t)op.b + (uint32_t)op.c + kConstSlack);
  const uint32_t cur = L.cur, end = L.end;
  L.cur = (uint32_t)op.b;
  L.end = (uint32_t)op.b + (uint32_t)op.c;
  Op o = op;
  o.b = 0; o.c = 0;
  if (op.code == OP_FIXED) h_fixed<EMIT, CAREFUL>(c, ks, L, o);
  else h_string<EMIT, CAREFUL>(c, ks, L, o);
  L.cur = cur;
  L.end = end;
}

// One op that carries a flag of this header, with a run-time Op (the generic interpreter)
template <bool EMIT, bool CAREFUL, class Ctx, class Src>
__device__ __forceinline__ void run_resolved(const Ctx& c, const Src& src, Lane& L, const Op& op) {
  if (op.flags & F_CONST) run_const<EMIT, CAREFUL>(c, src, L, op);
  else h_fixed_p<EMIT, CAREFUL>(c, src, L, op);
}

}  // namespace rh
#endif
