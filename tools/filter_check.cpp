// CPU check of pyruhvro_amd/csrc/filter_core.h (the twin of deflate_check.cpp: its own main, no HIP, no Python).
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I pyruhvro_amd/csrc \
//       tools/filter_check.cpp -o filter_check && ./filter_check
//
// 1. term_keeps_* against a plain restatement (the C++ operators, std::vector's lexicographic order), every kind x every
//    operator over the edge values: int64 min / max, +-0.0, NaN, +-inf, subnormals, float values widened, the empty string,
//    comparands equal to / a prefix of / longer than the value, bytes >= 0x80, 255-byte comparands, null.
// 2. The compaction arithmetic as the kernels use it (filter_kept, filter_len, filter_valid_mask, filter_rank_in_word,
//    filter_next_run; 256 records per block, 64 per word) against a plain concatenation of the kept records, for
//    n in {0, 1, 63, 64, 65, 256, 257} under the all / none / alternating / single-run masks and a few others.  Every buffer
//    sits in a heap block of exactly its size.
// Exit status 0 = no failure; the last line says what ran.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "filter_core.h"

using namespace rh;

static int failures = 0;
static size_t checks = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    checks++;                                             \
    if (!(cond)) {                                        \
      failures++;                                         \
      if (failures <= 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                     \
  } while (0)

static const char* const kOpName[] = {"==", "!=", "<", "<=", ">", ">=", "is_null", "not_null"};

// the plain restatement: nulls first, then the language's own operator
template <class T>
static bool ref_keeps(uint32_t op, bool isnull, const T& v, const T& k) {
  if (op == FC_IS_NULL) return isnull;
  if (op == FC_NOT_NULL) return !isnull;
  if (isnull) return false;
  switch (op) {
    case FC_EQ: return v == k;
    case FC_NE: return v != k;
    case FC_LT: return v < k;
    case FC_LE: return v <= k;
    case FC_GT: return v > k;
    default: return v >= k;
  }
}

static void check_ints() {
  const int64_t mn = std::numeric_limits<int64_t>::min(), mx = std::numeric_limits<int64_t>::max();
  const int64_t vals[] = {mn, mn + 1, -2147483649ll, -2147483648ll, -1, 0, 1, 127, 128, 2147483647ll, 2147483648ll, mx - 1, mx};
  for (int64_t v : vals)
    for (int64_t k : vals)
      for (uint32_t op = 0; op < 8; op++)
        for (int isnull = 0; isnull < 2; isnull++) {
          CHECK(term_keeps_int(op, isnull, v, k) == ref_keeps<int64_t>(op, isnull, v, k), "int %lld %s %lld null=%d", (long long)v, kOpName[op], (long long)k, isnull);
          CHECK(term_keeps_index(op, isnull, v, k) == ref_keeps<int64_t>(op, isnull, v, k), "index %lld %s %lld null=%d", (long long)v, kOpName[op], (long long)k, isnull);
        }
  // the 32-bit truncation of an int field's varint
  CHECK(filter_int32(0x100000000ll) == 0, "int32 of 2^32");
  CHECK(filter_int32(0xFFFFFFFFll) == -1, "int32 of 2^32 - 1");
  CHECK(filter_int32(-2147483648ll) == -2147483648ll, "int32 min");
  CHECK(filter_int32(2147483648ll) == -2147483648ll, "int32 of 2^31");
  CHECK(filter_int32(mn) == 0 && filter_int32(mx) == -1, "int32 of the int64 limits");
  // branch -> null
  CHECK(filter_branch_null(0, true) && !filter_branch_null(1, true) && !filter_branch_null(0, false) && filter_branch_null(1, false), "branch rule");
}

static void check_doubles() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double vals[] = {-inf, -std::numeric_limits<double>::max(), -1.5, -std::numeric_limits<double>::min(), -std::numeric_limits<double>::denorm_min(),
                         -0.0, 0.0, std::numeric_limits<double>::denorm_min(), std::numeric_limits<double>::min(), 1.0, 1.5,
                         (double)std::numeric_limits<float>::denorm_min(), (double)0.1f, 0.1, (double)std::numeric_limits<float>::max(),
                         9007199254740993.0, std::numeric_limits<double>::max(), inf, nan, -nan};
  for (double v : vals)
    for (double k : vals)
      for (uint32_t op = 0; op < 8; op++)
        for (int isnull = 0; isnull < 2; isnull++)
          CHECK(term_keeps_f64(op, isnull, v, k) == ref_keeps<double>(op, isnull, v, k), "double %g %s %g null=%d", v, kOpName[op], k, isnull);
  CHECK(term_keeps_f64(FC_EQ, false, -0.0, 0.0), "-0.0 == 0.0");
  CHECK(term_keeps_f64(FC_NE, false, nan, nan) && !term_keeps_f64(FC_EQ, false, nan, nan) && !term_keeps_f64(FC_LE, false, nan, 1.0), "NaN");
  CHECK(!term_keeps_f64(FC_NE, true, nan, 1.0), "null != x is false");
}

static void check_bools() {
  for (int v = 0; v < 2; v++)
    for (int k = 0; k < 2; k++)
      for (uint32_t op : {(uint32_t)FC_EQ, (uint32_t)FC_NE, (uint32_t)FC_IS_NULL, (uint32_t)FC_NOT_NULL})
        for (int isnull = 0; isnull < 2; isnull++)
          CHECK(term_keeps_index(op, isnull, v, k) == ref_keeps<int>(op, isnull, v, k), "bool %d %s %d null=%d", v, kOpName[op], k, isnull);
}

static void check_bytes() {
  std::vector<std::vector<uint8_t>> vals;
  auto S = [](const char* s) { return std::vector<uint8_t>(s, s + std::strlen(s)); };
  vals.push_back({});
  vals.push_back(S("a"));
  vals.push_back(S("ab"));
  vals.push_back(S("abc"));
  vals.push_back(S("abd"));
  vals.push_back(S("b"));
  vals.push_back({0x00});
  vals.push_back({0x7F});
  vals.push_back({0x80});
  vals.push_back({0xFF});
  vals.push_back({0x61, 0x80});
  vals.push_back({0x61, 0x00});
  vals.push_back({0xC3, 0xA9});                        // "é"
  vals.push_back(std::vector<uint8_t>(254, 'x'));
  vals.push_back(std::vector<uint8_t>(255, 'x'));
  vals.push_back(std::vector<uint8_t>(256, 'x'));       // (a value may be longer than any comparand)
  vals.push_back(std::vector<uint8_t>(1000, 'x'));
  { std::vector<uint8_t> y(255, 'x'); y[254] = 'y'; vals.push_back(y); }
  { std::vector<uint8_t> y(255, 0xFF); vals.push_back(y); }
  for (const auto& v : vals)
    for (const auto& k : vals) {
      if (k.size() > kMaxFilterBytes) continue;
      // exact heap blocks: a read past either end is an AddressSanitizer report
      std::unique_ptr<uint8_t[]> vb(new uint8_t[v.size()]), kb(new uint8_t[k.size()]);
      if (!v.empty()) std::memcpy(vb.get(), v.data(), v.size());
      if (!k.empty()) std::memcpy(kb.get(), k.data(), k.size());
      const uint8_t* vp = vb.get();
      const auto get = [vp](uint32_t i) { return (uint32_t)vp[i]; };
      const int c = bytes_order(get, v.size(), kb.get(), (uint32_t)k.size());
      CHECK(c == (v < k ? -1 : v > k ? 1 : 0), "bytes order, lengths %zu %zu", v.size(), k.size());
      for (uint32_t op = 0; op < 8; op++)
        for (int isnull = 0; isnull < 2; isnull++)
          CHECK(term_keeps_bytes(op, isnull, get, isnull ? 0 : v.size(), kb.get(), (uint32_t)k.size()) == ref_keeps<std::vector<uint8_t>>(op, isnull, v, k),
                "bytes %s, lengths %zu %zu null=%d", kOpName[op], v.size(), k.size(), isnull);
    }
}

// ---------------------------------------------------------------------------
// compaction: the kernels' steps in the kernels' order, on exact heap blocks
// ---------------------------------------------------------------------------
static void check_compaction(uint64_t n, const std::vector<bool>& mask, const char* what) {
  const uint64_t words = filter_words(n);
  std::unique_ptr<uint64_t[]> keep(new uint64_t[words]);
  for (uint64_t w = 0; w < words; w++) keep[w] = 0;
  for (uint64_t i = 0; i < n; i++)
    if (mask[i]) keep[i >> 6] |= 1ull << (i & 63);
  // records of 1 .. 40 bytes and a few over 64, every byte telling its record and its place
  std::unique_ptr<uint64_t[]> off(new uint64_t[n + 1]);
  off[0] = 0;
  for (uint64_t i = 0; i < n; i++) off[i + 1] = off[i] + (i % 29 == 7 ? 64 + i % 90 : 1 + (i * 7) % 40);
  std::unique_ptr<uint8_t[]> data(new uint8_t[off[n]]);
  for (uint64_t i = 0; i < n; i++)
    for (uint64_t b = off[i]; b < off[i + 1]; b++) data[b] = (uint8_t)(i * 131 + (b - off[i]) * 17 + 1);
  // the plain restatement
  std::vector<uint64_t> exp_off{0};
  std::vector<uint8_t> exp;
  for (uint64_t i = 0; i < n; i++)
    if (mask[i]) {
      exp.insert(exp.end(), data.get() + off[i], data.get() + off[i + 1]);
      exp_off.push_back(exp.size());
    }
  const uint64_t kept = exp_off.size() - 1;
  // rh_k_filter_lens: block sums
  const uint64_t nblocks = (n + kFilterBlock - 1) / kFilterBlock;
  std::unique_ptr<uint64_t[]> bc(new uint64_t[nblocks]), bb(new uint64_t[nblocks]);
  for (uint64_t b = 0; b < nblocks; b++) {
    bc[b] = bb[b] = 0;
    for (uint64_t t = 0; t < kFilterBlock; t++) {
      const uint64_t i = b * kFilterBlock + t;      // (threads past n ask too)
      bc[b] += filter_kept(keep.get(), n, i) ? 1 : 0;
      bb[b] += filter_len(keep.get(), off.get(), n, i);
    }
  }
  // rh_k_filter_scan: exclusive prefixes in place
  uint64_t cc = 0, cb = 0;
  for (uint64_t b = 0; b < nblocks; b++) {
    const uint64_t c = bc[b], y = bb[b];
    bc[b] = cc; bb[b] = cb;
    cc += c; cb += y;
  }
  CHECK(cc == kept, "%s n=%llu: kept %llu, expected %llu", what, (unsigned long long)n, (unsigned long long)cc, (unsigned long long)kept);
  // rh_k_filter_offsets
  std::unique_ptr<uint64_t[]> noff(new uint64_t[kept + 1]), wrank(new uint64_t[words]);
  for (uint64_t r = 0; r <= kept; r++) noff[r] = ~0ull;
  if (n == 0) noff[0] = 0;      // (no launch: the engine decodes an empty list)
  for (uint64_t b = 0; b < nblocks; b++) {
    uint64_t ic = 0, ib = 0;
    for (uint64_t t = 0; t < kFilterBlock; t++) {
      const uint64_t i = b * kFilterBlock + t;
      const uint64_t c = filter_kept(keep.get(), n, i) ? 1 : 0, v = filter_len(keep.get(), off.get(), n, i);
      ic += c; ib += v;
      if (c) noff[bc[b] + ic - 1] = bb[b] + ib - v;
      if (i < n && (i & 63) == 0) wrank[i >> 6] = bc[b] + ic - c;
      if (i + 1 == n) noff[bc[b] + ic] = bb[b] + ib;
    }
  }
  for (uint64_t r = 0; r <= kept; r++)
    CHECK(noff[r] == exp_off[r], "%s n=%llu: new_offsets[%llu] = %llu, expected %llu", what, (unsigned long long)n, (unsigned long long)r,
          (unsigned long long)noff[r], (unsigned long long)exp_off[r]);
  // rh_k_filter_gather: one word at a time, run by run
  std::unique_ptr<uint8_t[]> out(new uint8_t[exp.size()]);
  std::memset(out.get(), 0, exp.size());
  uint64_t copied = 0;
  for (uint64_t w = 0; w < words; w++) {
    const uint64_t r0 = w << 6;
    const uint32_t cnt = n - r0 < 64 ? (uint32_t)(n - r0) : 64u;
    const uint64_t word = keep[w] & filter_valid_mask(n, w);
    uint32_t j = 0, b, e;
    while (filter_next_run(word, j, cnt, &b, &e)) {
      CHECK(b >= j && b < e && e <= cnt, "%s n=%llu: run [%u, %u) of word %llu", what, (unsigned long long)n, b, e, (unsigned long long)w);
      for (uint32_t q = b; q < e; q++) CHECK((word >> q) & 1ull, "run holds a dropped record");
      CHECK(e == cnt || !((word >> e) & 1ull), "run ends in front of a kept record");
      for (uint32_t q = j; q < b; q++) CHECK(!((word >> q) & 1ull), "run skips a kept record");
      const uint64_t s0 = off[r0 + b], s1 = off[r0 + e];
      const uint64_t d0 = noff[wrank[w] + filter_rank_in_word(word, b)];
      if (d0 + (s1 - s0) <= exp.size()) std::memcpy(out.get() + d0, data.get() + s0, s1 - s0);
      else CHECK(false, "%s n=%llu: a run would be copied past the end", what, (unsigned long long)n);
      copied += s1 - s0;
      j = e;
    }
    for (uint32_t q = j; q < cnt; q++) CHECK(!((word >> q) & 1ull), "a kept record behind the last run");
  }
  CHECK(copied == exp.size(), "%s n=%llu: %llu bytes copied, expected %zu", what, (unsigned long long)n, (unsigned long long)copied, exp.size());
  CHECK(exp.empty() || std::memcmp(out.get(), exp.data(), exp.size()) == 0, "%s n=%llu: the gathered bytes differ", what, (unsigned long long)n);
}

static void check_compactions() {
  size_t cases = 0;
  for (uint64_t n : {0ull, 1ull, 63ull, 64ull, 65ull, 255ull, 256ull, 257ull, 1024ull, 1100ull}) {
    std::vector<bool> m(n);
    m.assign(n, true); check_compaction(n, m, "all"); cases++;
    m.assign(n, false); check_compaction(n, m, "none"); cases++;
    for (uint64_t i = 0; i < n; i++) m[i] = i % 2 == 0;
    check_compaction(n, m, "alternating"); cases++;
    for (uint64_t i = 0; i < n; i++) m[i] = i % 2 == 1;
    check_compaction(n, m, "alternating, odd"); cases++;
    m.assign(n, false);
    if (n) m[0] = true;
    check_compaction(n, m, "first only"); cases++;
    m.assign(n, false);
    if (n) m[n - 1] = true;
    check_compaction(n, m, "last only"); cases++;
    for (uint64_t i = 0; i < n; i++) m[i] = i >= n / 3 && i < n - n / 4;      // one run, across word and block edges
    check_compaction(n, m, "single run"); cases++;
    for (uint64_t i = 0; i < n; i++) m[i] = i >= 250 && i < 262;
    check_compaction(n, m, "run across a block edge"); cases++;
    uint64_t x = 88172645463325252ull;
    for (uint64_t i = 0; i < n; i++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; m[i] = (x & 7) < 3; }
    check_compaction(n, m, "random"); cases++;
  }
  std::printf("filter_check: %zu compaction cases\n", cases);
}

int main() {
  check_ints();
  check_doubles();
  check_bools();
  check_bytes();
  check_compactions();
  std::printf("filter_check: %zu checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
