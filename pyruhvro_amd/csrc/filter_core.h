// Row filters (rh_filter_*, rh_decode*_where): the compiled predicate, what a term keeps, and the arithmetic of the
// compaction.  Free of HIP and shared by the host (engine_filter.cpp, tools/filter_check.cpp) and the device (filter.hip), like
// call_plan.h and deflate_core.h: the null, NaN and bytewise rules are stated here once and nowhere else.  Not one of the headers
// the specialised kernels include: the kernel-cache key does not see this file.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RF_HD __host__ __device__
#else
#define RF_HD
#endif

namespace rh {

constexpr uint32_t kMaxFilterTerms = 8;
constexpr uint32_t kMaxFilterBytes = 255;      // a byte comparand (kMaxDefaultBytes of the resolver)

// how the value of a marked op is read and compared
enum FilterKind : uint32_t {
  FLT_I32 = 0,   // int / date / time-millis: a varint, truncated to 32 bits as the decode truncates it, compared as int64
  FLT_I64,       // long and its logical types: a varint
  FLT_F32,       // 4 raw bytes, widened to double
  FLT_F64,       // 8 raw bytes
  FLT_BOOL,      // 1 raw byte
  FLT_BYTES,     // string / bytes: a length and that many bytes, unsigned bytewise lexicographic order
  FLT_ENUM,      // a varint index, compared with the comparand symbol's index
};

enum FilterCmp : uint32_t { FC_EQ = 0, FC_NE, FC_LT, FC_LE, FC_GT, FC_GE, FC_IS_NULL, FC_NOT_NULL };

struct FilterTerm {
  int32_t pc;        // the op of the writer's plain program that decodes the field (OP_FIXED / OP_STRING / OP_ENUM, domain 0)
  uint32_t kind;     // FilterKind
  uint32_t cmp;      // FilterCmp
  uint32_t blen;     // FLT_BYTES: bytes of the comparand
  uint32_t boff;     // ... and where they start in the predicate's byte blob
  uint32_t pad;
  int64_t i;         // FLT_I32 / FLT_I64 / FLT_ENUM (symbol index) / FLT_BOOL (0 or 1)
  double d;          // FLT_F32 / FLT_F64
};

struct FilterProgram {
  uint32_t nterms;   // 1 .. kMaxFilterTerms, ANDed
  uint32_t pad;
  FilterTerm term[kMaxFilterTerms];
};

// ---------------------------------------------------------------------------
// what a term keeps.  A null value fails every comparison, != included; is_null / not_null are the only terms that look at
// nothing else.  (A non-nullable field is never null: is_null keeps nothing, not_null everything.)
// ---------------------------------------------------------------------------
// `c`: the order of value against comparand (-1, 0, 1); `unordered`: there is none (a NaN on either side)
RF_HD inline bool cmp_keeps(uint32_t cmp, int c, bool unordered) {
  switch (cmp) {
    case FC_EQ: return !unordered && c == 0;
    case FC_NE: return unordered || c != 0;       // IEEE: NaN != x is true
    case FC_LT: return !unordered && c < 0;
    case FC_LE: return !unordered && c <= 0;
    case FC_GT: return !unordered && c > 0;
    case FC_GE: return !unordered && c >= 0;
    default: return false;
  }
}
RF_HD inline bool null_rule(uint32_t cmp, bool isnull, bool* decided) {
  *decided = true;
  if (cmp == FC_IS_NULL) return isnull;
  if (cmp == FC_NOT_NULL) return !isnull;
  if (isnull) return false;
  *decided = false;
  return false;
}
RF_HD inline bool term_keeps_int(uint32_t cmp, bool isnull, int64_t v, int64_t k) {
  bool done;
  const bool r = null_rule(cmp, isnull, &done);
  if (done) return r;
  return cmp_keeps(cmp, v < k ? -1 : v > k ? 1 : 0, false);
}
// float / double, the float already widened: IEEE order, -0.0 == 0.0, NaN unordered
RF_HD inline bool term_keeps_f64(uint32_t cmp, bool isnull, double v, double k) {
  bool done;
  const bool r = null_rule(cmp, isnull, &done);
  if (done) return r;
  const bool un = v != v || k != k;
  return cmp_keeps(cmp, un ? 0 : v < k ? -1 : v > k ? 1 : 0, un);
}
// boolean and enum index: == / != (the front end refuses the other four)
RF_HD inline bool term_keeps_index(uint32_t cmp, bool isnull, int64_t v, int64_t k) { return term_keeps_int(cmp, isnull, v, k); }
// string / bytes: `get(i)` returns byte i of the value (only asked for i < vlen), `k` the comparand.  Unsigned bytewise order; a
// proper prefix sorts first.  The loop runs klen times whatever the value is: on the device its trip count is wave-uniform.
template <class Get>
RF_HD inline int bytes_order(const Get& get, uint64_t vlen, const uint8_t* k, uint32_t klen) {
  int c = 0;
  for (uint32_t i = 0; i < klen; i++) {
    if (c == 0 && (uint64_t)i < vlen) {
      const uint32_t b = get(i) & 0xFFu, kb = k[i];
      c = b < kb ? -1 : b > kb ? 1 : 0;
    }
  }
  if (c == 0) c = vlen < (uint64_t)klen ? -1 : vlen > (uint64_t)klen ? 1 : 0;
  return c;
}
template <class Get>
RF_HD inline bool term_keeps_bytes(uint32_t cmp, bool isnull, const Get& get, uint64_t vlen, const uint8_t* k, uint32_t klen) {
  bool done;
  const bool r = null_rule(cmp, isnull, &done);
  if (done) return r;
  return cmp_keeps(cmp, bytes_order(get, vlen, k, klen), false);
}

// the 32-bit truncation of an int field's varint (walk.h varint35 / fast_decode.rs `as i32`), sign-extended
RF_HD inline int64_t filter_int32(int64_t v) { return (int64_t)(int32_t)(uint32_t)(uint64_t)v; }
// branch index of a [null, T] / [T, null] union -> the value is null
RF_HD inline bool filter_branch_null(int64_t idx, bool null_first) { return (idx == 0) == null_first; }

// ---------------------------------------------------------------------------
// compaction: record i with keep bit set goes to rank(i) = the kept records in front of it, at byte new_offsets[rank(i)] =
// the kept bytes in front of it; new_offsets[kept] = all kept bytes.  One keep word per 64 records, bit j = record 64 w + j.
// ---------------------------------------------------------------------------
constexpr uint32_t kFilterBlock = 256;      // records per workgroup of the length / offset kernels (four keep words)

RF_HD inline uint64_t filter_words(uint64_t n) { return (n + 63) / 64; }
// the bits of word w that belong to records below n
RF_HD inline uint64_t filter_valid_mask(uint64_t n, uint64_t w) {
  const uint64_t r0 = w << 6;
  if (r0 >= n) return 0;
  const uint64_t cnt = n - r0;
  return cnt >= 64 ? ~0ull : ((1ull << cnt) - 1ull);
}
RF_HD inline bool filter_kept(const uint64_t* keep, uint64_t n, uint64_t i) { return i < n && ((keep[i >> 6] >> (i & 63)) & 1ull); }
RF_HD inline uint32_t filter_popc(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popcll(x);
#else
  return (uint32_t)__builtin_popcountll(x);
#endif
}
RF_HD inline uint32_t filter_ctz(uint64_t x) {      // x != 0
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__ffsll((unsigned long long)x) - 1u;
#else
  return (uint32_t)__builtin_ctzll(x);
#endif
}
// kept records of the word in front of bit j (j < 64)
RF_HD inline uint32_t filter_rank_in_word(uint64_t word, uint32_t j) { return filter_popc(word & ((1ull << j) - 1ull)); }
// what record i adds to the two prefix sums
RF_HD inline uint64_t filter_len(const uint64_t* keep, const uint64_t* offsets, uint64_t n, uint64_t i) {
  return filter_kept(keep, n, i) ? offsets[i + 1] - offsets[i] : 0;
}
// The next run of kept neighbours of a word at or behind bit j: false when there is none, else [*b, *e) with e <= cnt.  `word` is
// already cut to its cnt valid bits.  The gather copies a run in one go: its records are contiguous in source and destination.
RF_HD inline bool filter_next_run(uint64_t word, uint32_t j, uint32_t cnt, uint32_t* b, uint32_t* e) {
  if (j >= cnt) return false;
  const uint64_t rest = word >> j;
  if (!rest) return false;
  const uint32_t s = j + filter_ctz(rest);
  const uint64_t gaps = ~(word >> s);               // first dropped record at or behind s
  const uint32_t len = gaps ? filter_ctz(gaps) : 64u;
  *b = s;
  *e = s + len < cnt ? s + len : cnt;
  return true;
}

}  // namespace rh
