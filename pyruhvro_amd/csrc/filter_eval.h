// Row filters on the device: reading a marked field's value back and applying the predicate's terms to it.
// Shared by the two kernels that evaluate a predicate inside a careful walk -- rh_k_filter (filter.hip: one lane per record) and
// rh_k_split_where (container.hip: one lane per container block) -- so that both compile from the same text.  Include it behind
// walk.h (varint64, the sources).  Not one of the headers the specialised kernels include: the kernel-cache key does not see
// this file.
#pragma once
#include "program.h"
#include "filter_core.h"

namespace rh {

typedef const __attribute__((address_space(4))) Op* FProgPtr;
__device__ __forceinline__ Op f_ld_op(FProgPtr p) {
  Op o;
  o.code = p->code; o.flags = p->flags; o.dom = p->dom; o.a = p->a; o.b = p->b; o.c = p->c;
  o.buf0 = p->buf0; o.buf1 = p->buf1; o.buf2 = p->buf2; o.node = p->node;
  return o;
}

// Which ops the terms mark, held in scalar registers for the whole walk: the test runs at EVERY op of every record, and a walk
// that is one dependent chain per lane (rh_k_split_where: a wavefront per 64 blocks) pays for every scalar load of a term's pc
// from the kernel arguments in full.  readfirstlane makes each value a register definition the compiler cannot re-load in the loop.
struct FMarks {
  int lo, hi;                      // no term marks an op outside [lo, hi]
  int pc[kMaxFilterTerms];         // -1: no such term
};
__device__ __forceinline__ FMarks f_marks(const FilterProgram& flt) {
  FMarks m;
  m.lo = 0x7FFFFFFF; m.hi = -1;
#pragma unroll
  for (uint32_t t = 0; t < kMaxFilterTerms; t++) {
    const int pc = t < flt.nterms ? flt.term[t].pc : -1;
    m.pc[t] = __builtin_amdgcn_readfirstlane(pc);
    if (pc >= 0) { m.lo = pc < m.lo ? pc : m.lo; m.hi = pc > m.hi ? pc : m.hi; }
  }
  m.lo = __builtin_amdgcn_readfirstlane(m.lo);
  m.hi = __builtin_amdgcn_readfirstlane(m.hi);
  return m;
}
// the terms that mark the op at `pc` (wave-uniform: pc is, and so are the marks)
__device__ __forceinline__ uint32_t f_terms_at(const FMarks& m, int pc) {
  uint32_t tm = 0;
  if (pc >= m.lo && pc <= m.hi) {
#pragma unroll
    for (uint32_t t = 0; t < kMaxFilterTerms; t++)
      if (m.pc[t] == pc) tm |= 1u << t;
  }
  return tm;
}

// A varint the careful walk has accepted, read again at p: its value and its bytes.  Up to 8 bytes in one read; a longer or
// padded one byte by byte, ten turns whatever the bytes are (the tenth byte gives bit 63 only, as the walk reads it).
template <class Src>
__device__ __forceinline__ uint32_t f_varint(const Src& src, uint32_t p, bool act, int64_t& v) {
  uint32_t n = 1;
  v = 0;
  const bool ok = varint64(src.ld8(p), 8, 0x7FFFFFFFu, v, n);
  if (__any(act && !ok)) {
    if (act && !ok) {
      uint64_t r = 0;
      bool done = false;
      n = 0;
      for (uint32_t k = 0; k < 10; k++) {
        if (!done) {
          const uint32_t b = src.ld1(p + k);
          r |= (uint64_t)(b & 0x7Fu) << (7u * k);
          n = k + 1;
          done = (b & 0x80u) == 0;
        }
      }
      v = (int64_t)(r >> 1) ^ -(int64_t)(r & 1);
    }
  }
  return n;
}

// The terms `tm` (a wave-uniform bit set) of the field whose bytes start at p, for the lanes with `act` (a record, no error).
// `flt` is a pointer on purpose: where it points into device memory (rh_k_split_where) the terms' fields are loaded HERE, at a
// marked op, and not hoisted in front of the walk -- 64 scalars held across the walk loop spill its own state (measured).
// A lane without `act` runs the same reads at whatever p it holds: the source bounds them, and its result means nothing.
template <class Src>
__device__ __forceinline__ bool f_eval(const FilterProgram* flt, const uint8_t* cbytes, const Src& src, const Op& op, uint32_t tm, uint32_t p, bool act) {
  uint32_t kind = 0;
#pragma unroll
  for (uint32_t t = 0; t < kMaxFilterTerms; t++)
    if ((tm >> t) & 1u) kind = flt->term[t].kind;      // (every term of one field has the field's kind)
  bool isnull = false;
  if (op.flags & F_NULLABLE) {
    int64_t idx = 0;
    p += f_varint(src, p, act, idx);
    isnull = filter_branch_null(idx, (op.flags & F_NULL_FIRST) != 0);
  }
  const bool val = act && !isnull;
  int64_t iv = 0;
  double dv = 0.0;
  uint64_t vlen = 0;
  uint32_t vpos = p;
  switch (kind) {      // (wave-uniform)
    case FLT_I32: case FLT_I64: case FLT_ENUM: {
      int64_t x = 0;
      f_varint(src, p, val, x);
      iv = kind == FLT_I32 ? filter_int32(x) : x;
      break;
    }
    case FLT_F32: dv = (double)__uint_as_float(src.ld4(p)); break;
    case FLT_F64: dv = __longlong_as_double((long long)src.ld8(p)); break;
    case FLT_BOOL: iv = (src.ld1(p) & 0xFFu) != 0 ? 1 : 0; break;
    default: {           // FLT_BYTES
      int64_t len = 0;
      const uint32_t nb = f_varint(src, p, val, len);
      vlen = val ? (uint64_t)len : 0ull;
      vpos = p + nb;
      break;
    }
  }
  bool keep = true;
#pragma unroll
  for (uint32_t t = 0; t < kMaxFilterTerms; t++) {
    if (!((tm >> t) & 1u)) continue;
    const uint32_t cmp = flt->term[t].cmp;
    bool k;
    switch (kind) {
      case FLT_I32: case FLT_I64: k = term_keeps_int(cmp, isnull, iv, flt->term[t].i); break;
      case FLT_ENUM: case FLT_BOOL: k = term_keeps_index(cmp, isnull, iv, flt->term[t].i); break;
      case FLT_F32: case FLT_F64: k = term_keeps_f64(cmp, isnull, dv, flt->term[t].d); break;
      default: {
        const auto get = [src, vpos](uint32_t i) { return src.ld1(vpos + i); };      // (asked for i < vlen only: inside the value)
        k = term_keeps_bytes(cmp, isnull, get, vlen, cbytes + flt->term[t].boff, flt->term[t].blen);
        break;
      }
    }
    keep = keep && k;
  }
  return keep;
}

// The program, every op counters-only and careful (walk_drop.h run_dropped), with the predicate evaluated at the ops its terms
// mark: the lane notes its cursor, runs the op, and while it is still error-free reads the value back.  Returns whether the
// lane's record matches (`mine`: the lane has a record; `marks`: f_marks(flt), made once per kernel).  Ctx: what DropCtx needs of the walk's context.
template <class Ctx, class Src>
__device__ __forceinline__ bool filter_walk(const Op* program, const FilterProgram* flt, const FMarks& marks, const uint8_t* cbytes, const Ctx& c, const Src& src,
                                            Lane& L, bool mine) {
  const FProgPtr prog = reinterpret_cast<FProgPtr>(reinterpret_cast<uintptr_t>(program));
  bool keep = mine;
  int pc = 0;
  for (;;) {
    pc = __builtin_amdgcn_readfirstlane(pc);
    const Op op = f_ld_op(prog + pc);
    if (op.code == OP_END) return keep;
    int npc = op.code == OP_LIST_TAIL ? op.b : pc + 1;      // LIST_TAIL goes back to its LIST_NEXT
    if (op.code > OP_BIN) return keep;
    const uint32_t tm = f_terms_at(marks, pc);                // the terms that mark this op (wave-uniform)
    const uint32_t cur0 = L.cur;
    if (!run_dropped<false, true>(c, src, L, op)) npc = op.b;      // no lane has an item left: to LIST_END
    if (tm) {
      const bool k = f_eval(flt, cbytes, src, op, tm, cur0, mine && L.err == 0);
      keep = keep && k;
    }
    pc = npc;
  }
}

}  // namespace rh
