// CPU check of pyruhvro_amd/csrc/frame_join_core.h (the twin of frame_check.cpp: its own main, no HIP, no Python).
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I pyruhvro_amd/csrc
//       tools/frame_join_check.cpp -o frame_join_check && ./frame_join_check
//
// 1. join_header_byte for every id edge of tests/frame_cases.py (CONFLUENT_EDGES, SINGLE_EDGES), read back with frame_core.h's own
//    frame_marker_ok / frame_id and compared with bytes written out per framing.
// 2. The copy of one message as a 16-lane group of rh_k_join_gather runs it, for every destination alignment 0 .. 15, every datum
//    length 0 .. 80 and 255, 256, 257, both framings: vector stores aligned on the destination, no byte read outside the datum, no
//    byte written outside the message, every byte of the message written exactly once.
// 3. The join as the kernels run it (frame_join.hip: lengths, tile sums, scan 256 tiles a round with a carry, offsets, gather)
//    against std::partial_sum and plain loops, for n in {0, 1, 63, 64, 65, 255, 256, 257, 1024, 1100} and for 257 tiles, with and
//    without indices, several chunk counts, sources of no rows among the sources.
// 4. The permutation's verdicts: a position named twice, a hole, an index out of range, each in the first and in the last tile.
// Every buffer sits in a heap block of exactly its size.  Exit status 0 = no failure; the last line says what ran.
#include <cstdio>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

#include "frame_join_core.h"

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

// ---------------------------------------------------------------------------
// the plain restatement
// ---------------------------------------------------------------------------
static std::vector<uint8_t> plain_header(uint32_t kind, uint64_t id) {
  std::vector<uint8_t> m;
  if (kind == FRAME_CONFLUENT) {
    m = {0x00, (uint8_t)(id >> 24), (uint8_t)(id >> 16), (uint8_t)(id >> 8), (uint8_t)id};
  } else {
    m = {0xC3, 0x01};
    for (int i = 0; i < 8; i++) m.push_back((uint8_t)(id >> (8 * i)));
  }
  return m;
}

static const uint64_t kConfluentEdges[] = {0, 1, 0x01000000ull, 0x7FFFFFFFull, 0x80000000ull, 0xFFFFFFFFull};
static const uint64_t kSingleEdges[] = {0x1122334455667700ull, 0x1122334455667701ull, 0x9122334455667700ull, 0, 0x8000000000000000ull, ~0ull};

static void check_headers() {
  for (uint32_t kind = 0; kind < FRAME_KINDS; kind++) {
    const FrameDesc d = frame_desc(kind);
    const uint64_t* edges = kind == FRAME_CONFLUENT ? kConfluentEdges : kSingleEdges;
    for (uint32_t e = 0; e < 6; e++) {
      const uint64_t id = edges[e];
      std::unique_ptr<uint8_t[]> blk(new uint8_t[d.header]);
      for (uint32_t i = 0; i < d.header; i++) blk[i] = join_header_byte(d, id, i);
      const std::vector<uint8_t> want = plain_header(kind, id);
      CHECK(want.size() == d.header && std::memcmp(blk.get(), want.data(), d.header) == 0, "framing %u: the header of id %llx", kind, (unsigned long long)id);
      CHECK(frame_marker_ok(blk.get(), d), "framing %u: the marker of id %llx", kind, (unsigned long long)id);
      CHECK(frame_id(blk.get(), d) == id, "framing %u: id %llx reads back as %llx", kind, (unsigned long long)id, (unsigned long long)frame_id(blk.get(), d));
    }
  }
}

// ---------------------------------------------------------------------------
// one message by one 16-lane group: jn_group_message of frame_join.hip, lane by lane.  `dst_addr` stands for the destination's
// address; out is an exact block of header + len bytes, s one of len bytes.  wrote[i] counts the writes of byte i.
// ---------------------------------------------------------------------------
static void group_message(uint8_t* out, uint64_t dst_addr, const uint8_t* s, uint64_t len, uint64_t id, const FrameDesc& d, std::vector<uint32_t>& wrote,
                          const char* what) {
  const uint64_t total = d.header + len;
  auto put = [&](uint64_t at, uint8_t b) {
    if (at >= total) { CHECK(false, "%s: a byte written outside the message", what); return; }
    out[at] = b;
    wrote[at]++;
  };
  auto get = [&](uint64_t at) -> uint8_t {
    if (at >= len) { CHECK(false, "%s: a byte read outside the datum", what); return 0; }
    return s[at];
  };
  const FrameCopy c = join_copy_plan(dst_addr, d, len);
  CHECK(c.head + 16 * c.nvec + c.tail == len && c.head < 16 && c.tail < 16, "%s: the plan does not cover the datum", what);
  CHECK(c.nvec == 0 || (dst_addr + d.header + c.head) % 16 == 0, "%s: the vector stores are not aligned on the destination", what);
  for (uint32_t sub = 0; sub < kFrameGroup; sub++) {
    if (sub < d.header) put(sub, join_header_byte(d, id, sub));
    if (!len) continue;
    if (sub < c.head) put(d.header + sub, get(sub));
    for (uint64_t v = sub; v < c.nvec; v += kFrameGroup)
      for (uint32_t b = 0; b < 16; b++) put(d.header + c.head + (v << 4) + b, get(c.head + (v << 4) + b));
    const uint64_t done = c.head + (c.nvec << 4);
    if (sub < c.tail) put(d.header + done + sub, get(done + sub));
  }
}

static void check_copy_plan() {
  std::vector<uint64_t> lens;
  for (uint64_t l = 0; l <= 80; l++) lens.push_back(l);
  for (uint64_t l : {255ull, 256ull, 257ull}) lens.push_back(l);
  size_t cases = 0;
  for (uint32_t kind = 0; kind < FRAME_KINDS; kind++) {
    const FrameDesc d = frame_desc(kind);
    const uint64_t id = kind == FRAME_CONFLUENT ? 0x01020304ull : 0x1122334455667788ull;
    CHECK(d.header <= kFrameGroup, "framing %u: a group has a lane for every header byte", kind);
    for (uint64_t align = 0; align < 16; align++)
      for (uint64_t len : lens) {
        std::unique_ptr<uint8_t[]> s(new uint8_t[len]);
        for (uint64_t b = 0; b < len; b++) s[b] = (uint8_t)(b * 37 + align + 1);
        std::unique_ptr<uint8_t[]> out(new uint8_t[d.header + len]);
        std::memset(out.get(), 0xEE, d.header + len);
        std::vector<uint32_t> wrote(d.header + len, 0);
        const std::string what = std::string(kind ? "single_object" : "confluent") + ", alignment " + std::to_string(align) + ", " + std::to_string(len) + " bytes";
        group_message(out.get(), 0x7000 + align, s.get(), len, id, d, wrote, what.c_str());
        std::vector<uint8_t> want = plain_header(kind, id);
        want.insert(want.end(), s.get(), s.get() + len);
        CHECK(std::memcmp(out.get(), want.data(), want.size()) == 0, "%s: the message differs", what.c_str());
        bool once = true;
        for (uint32_t w : wrote) once = once && w == 1;
        CHECK(once, "%s: a byte was not written exactly once", what.c_str());
        cases++;
      }
  }
  std::printf("frame_join_check: %zu copy cases\n", cases);
}

// ---------------------------------------------------------------------------
// the join: the kernels' steps in the kernels' order, on exact heap blocks
// ---------------------------------------------------------------------------
struct Src {
  uint64_t id;
  std::vector<std::vector<uint8_t>> datums;
  std::unique_ptr<int32_t[]> off;
  std::unique_ptr<uint8_t[]> data;
  uint64_t bytes = 0;
};

static size_t datum_len(uint64_t i) {      // 0 (the bare header), the lengths around a vector, a few long ones
  static const size_t kLens[] = {0, 1, 15, 16, 17, 31, 33, 2, 7, 40};
  return i % 37 == 9 ? 64 + i % 90 : i % 101 == 50 ? 700 : kLens[i % 10];
}

struct Outcome {
  uint64_t bad_range = kJoinNone;      // the lowest source row whose index is out of range
  JoinVerdict verdict = JOIN_OK;
  uint64_t at = 0;
  bool ran = false;                    // the gather ran: out / off hold the result
  std::vector<std::vector<int32_t>> off;
  std::vector<std::vector<uint8_t>> out;
};

// rows[s]: the rows of source s; indices: empty = none, else one per row over all sources in order
static Outcome run_join(uint32_t kind, const std::vector<uint64_t>& rows, const std::vector<int64_t>& indices, uint64_t num_chunks, const char* what) {
  const FrameDesc d = frame_desc(kind);
  Outcome R;
  // ---- the sources, as encode results hold them: i32 offsets + data, exactly sized; sources of no rows are left out of the table
  std::vector<Src> srcs(rows.size());
  uint64_t n = 0, g = 0;
  for (size_t s = 0; s < rows.size(); s++) {
    srcs[s].id = kind == FRAME_CONFLUENT ? kConfluentEdges[s % 6] + 16 * (s / 6) : kSingleEdges[s % 6] + 2 * (s / 6);
    srcs[s].off.reset(new int32_t[rows[s] + 1]);
    srcs[s].off[0] = 0;
    for (uint64_t j = 0; j < rows[s]; j++, g++) {
      std::vector<uint8_t> dat(datum_len(g));
      for (size_t b = 0; b < dat.size(); b++) dat[b] = (uint8_t)(g * 131 + b * 17 + 1);
      srcs[s].off[j + 1] = srcs[s].off[j] + (int32_t)dat.size();
      srcs[s].datums.push_back(dat);
    }
    srcs[s].bytes = (uint64_t)srcs[s].off[rows[s]];
    srcs[s].data.reset(new uint8_t[srcs[s].bytes]);
    for (uint64_t j = 0; j < rows[s]; j++)
      if (!srcs[s].datums[j].empty()) std::memcpy(srcs[s].data.get() + srcs[s].off[j], srcs[s].datums[j].data(), srcs[s].datums[j].size());
    n += rows[s];
  }
  std::vector<JoinSource> tab;
  uint64_t end = 0;
  for (size_t s = 0; s < rows.size(); s++) {
    if (!rows[s]) continue;
    end += rows[s];
    tab.push_back(JoinSource{srcs[s].off.get(), srcs[s].data.get(), end, srcs[s].id, srcs[s].bytes});
  }
  const uint32_t m = (uint32_t)tab.size();
  std::unique_ptr<JoinSource[]> table(new JoinSource[m]);
  for (uint32_t t = 0; t < m; t++) table[t] = tab[t];
  const uint32_t turns = join_search_turns(m);
  const bool with = !indices.empty();
  const uint32_t k = (uint32_t)(num_chunks < 1 ? 1 : num_chunks > (n ? n : 1) ? (n ? n : 1) : num_chunks);      // rh_clamp_chunks
  const uint64_t sz = n / k;
  if (n == 0) { R.ran = true; R.off.assign(1, std::vector<int32_t>{0}); R.out.assign(1, {}); return R; }      // (no launch)

  // ---- rh_k_join_lengths
  const uint64_t ntiles = join_tiles(n);
  std::unique_ptr<uint32_t[]> claim(new uint32_t[join_claim_words(n)]);
  std::memset(claim.get(), 0, 4 * join_claim_words(n));
  std::unique_ptr<uint32_t[]> len(new uint32_t[n]), who(new uint32_t[n]);
  std::unique_ptr<const uint8_t*[]> at(new const uint8_t*[n]);
  for (uint64_t p = 0; p < n; p++) { len[p] = 0; who[p] = ~0u; at[p] = nullptr; }
  uint64_t bad_range = kJoinNone, bad_twice = kJoinNone;
  for (uint64_t r = 0; r < n; r++) {
    const uint32_t s = join_source_of(table.get(), m, r, turns);
    CHECK(s < m && table[s].row_end > r && (s == 0 || table[s - 1].row_end <= r), "%s: row %llu found in source %u", what, (unsigned long long)r, s);
    if (s >= m) return R;
    const uint64_t j = join_row_in_source(table.get(), s, r);
    const int64_t o0 = table[s].off[j], o1 = table[s].off[j + 1];
    uint64_t p = r;
    if (with) {
      const int64_t v = indices[r];
      if (!join_in_range(v, n)) { if (r < bad_range) bad_range = r; continue; }
      p = (uint64_t)v;
      const uint32_t bit = join_claim_bit(p);
      uint32_t& w = claim[join_claim_word(p)];
      if (w & bit) { if (p < bad_twice) bad_twice = p; }
      w |= bit;
    }
    len[p] = d.header + (uint32_t)(o1 - o0);
    who[p] = s;
    at[p] = table[s].data + o0;
  }
  // ---- rh_k_join_tile_sums, rh_k_join_scan (256 tiles a round with a carry), rh_k_join_offsets
  std::unique_ptr<uint64_t[]> tile_sum(new uint64_t[ntiles]), tile_pre(new uint64_t[ntiles]), pre(new uint64_t[n + 1]), base(new uint64_t[k + 1]);
  for (uint64_t t = 0; t < ntiles; t++) {
    uint64_t sum = 0;
    for (uint32_t i = 0; i < kJoinTile; i++) sum += t * kJoinTile + i < n ? len[t * kJoinTile + i] : 0;
    tile_sum[t] = sum;
  }
  uint64_t carry = 0;
  for (uint64_t b0 = 0; b0 < ntiles; b0 += kJoinTile) {
    uint64_t run = 0;
    for (uint32_t i = 0; i < kJoinTile; i++) {
      const uint64_t t = b0 + i;
      const uint64_t v = t < ntiles ? tile_sum[t] : 0;
      run += v;
      if (t < ntiles) tile_pre[t] = carry + run - v;
    }
    carry += run;
  }
  pre[n] = carry;
  base[k] = carry;
  for (uint64_t t = 0; t < ntiles; t++) {
    uint64_t incl = 0;
    for (uint32_t i = 0; i < kJoinTile; i++) {
      const uint64_t p = t * kJoinTile + i;
      if (p >= n) break;
      incl += len[p];
      pre[p] = tile_pre[t] + incl - len[p];
      if (join_opens_chunk(p, sz, k)) base[p / sz] = pre[p];
    }
  }
  // ---- the host's one look: the verdicts (the bitmap is read only when a position was named twice)
  R.bad_range = bad_range;
  if (bad_range != kJoinNone) return R;
  if (with) {
    const uint64_t never = bad_twice != kJoinNone ? join_lowest_hole(claim.get(), n) : kJoinNone;
    R.verdict = join_perm_verdict(bad_twice, never, &R.at);
    if (R.verdict != JOIN_OK) return R;
  }
  {      // the prefix against std::partial_sum
    std::vector<uint64_t> l(len.get(), len.get() + n), want(n);
    std::partial_sum(l.begin(), l.end(), want.begin());
    bool same = pre[0] == 0 && pre[n] == want[n - 1];
    for (uint64_t p = 1; p < n; p++) same = same && pre[p] == want[p - 1];
    CHECK(same, "%s n=%llu: the prefix differs from std::partial_sum", what, (unsigned long long)n);
  }
  // ---- the leases: per chunk offsets and data, exactly sized
  R.off.resize(k);
  R.out.resize(k);
  std::vector<std::unique_ptr<int32_t[]>> coff(k);
  std::vector<std::unique_ptr<uint8_t[]>> cdat(k);
  std::vector<uint64_t> crows(k), ctot(k);
  for (uint32_t c = 0; c < k; c++) {
    crows[c] = c == k - 1 ? n - (uint64_t)(k - 1) * sz : sz;
    ctot[c] = base[c + 1] - base[c];
    coff[c].reset(new int32_t[crows[c] + 1]);
    for (uint64_t r = 0; r <= crows[c]; r++) coff[c][r] = -1;
    cdat[c].reset(new uint8_t[ctot[c]]);
    std::memset(cdat[c].get(), 0xEE, ctot[c]);
  }
  // ---- rh_k_join_gather: a wavefront per 64 messages, 16 rounds of four 16-lane groups
  for (uint64_t r0 = 0; r0 < n; r0 += 64) {
    for (uint32_t lane = 0; lane < 64; lane++) {
      const uint64_t p = r0 + lane;
      if (p >= n) continue;
      const uint32_t c = join_chunk_of(p, sz, k);
      const uint64_t row = p - join_chunk_start(c, sz);
      if (row >= crows[c]) { CHECK(false, "%s: message %llu lands past chunk %u", what, (unsigned long long)p, c); continue; }
      coff[c][row] = (int32_t)(pre[p] - base[c]);
      if (join_closes_chunk(p, n, sz, k)) {
        CHECK(row + 1 == crows[c], "%s: message %llu closes chunk %u at row %llu", what, (unsigned long long)p, c, (unsigned long long)row);
        coff[c][row + 1] = (int32_t)(pre[p + 1] - base[c]);
      }
    }
    for (uint32_t round = 0; round < kFrameRounds; round++)
      for (uint32_t group = 0; group < kFrameGroups; group++) {
        const uint64_t p = r0 + kFrameGroups * round + group;
        if (p >= n) continue;
        const uint32_t c = join_chunk_of(p, sz, k);
        const uint64_t to = pre[p] - base[c], dl = len[p] - d.header;
        if (to + len[p] > ctot[c]) { CHECK(false, "%s: message %llu would be written past chunk %u", what, (unsigned long long)p, c); continue; }
        std::vector<uint32_t> wrote(len[p], 0);
        // (the chunk's data starts 16-byte aligned, as a lease's does: the offset stands for the address)
        group_message(cdat[c].get() + to, to, at[p], dl, table[who[p]].id, d, wrote, what);
      }
  }
  for (uint32_t c = 0; c < k; c++) {
    R.off[c].assign(coff[c].get(), coff[c].get() + crows[c] + 1);
    R.out[c].assign(cdat[c].get(), cdat[c].get() + ctot[c]);
  }
  R.ran = true;
  // ---- against the plain restatement: message p is header(id of its group) + datum, the chunks as rh_encode cuts n rows
  std::vector<std::vector<uint8_t>> msgs(n);
  uint64_t r = 0;
  for (size_t s = 0; s < rows.size(); s++)
    for (uint64_t j = 0; j < rows[s]; j++, r++) {
      std::vector<uint8_t> msg = plain_header(kind, srcs[s].id);
      msg.insert(msg.end(), srcs[s].datums[j].begin(), srcs[s].datums[j].end());
      msgs[with ? (uint64_t)indices[r] : r] = msg;
    }
  for (uint32_t c = 0; c < k; c++) {
    std::vector<int32_t> woff{0};
    std::vector<uint8_t> wdat;
    for (uint64_t q = 0; q < crows[c]; q++) {
      const std::vector<uint8_t>& msg = msgs[(uint64_t)c * sz + q];
      wdat.insert(wdat.end(), msg.begin(), msg.end());
      woff.push_back((int32_t)wdat.size());
    }
    CHECK(R.off[c] == woff, "%s n=%llu k=%u: the offsets of chunk %u differ", what, (unsigned long long)n, k, c);
    CHECK(R.out[c] == wdat, "%s n=%llu k=%u: the bytes of chunk %u differ", what, (unsigned long long)n, k, c);
  }
  return R;
}

// the rows of n messages dealt to `m` sources in runs, with sources of no rows at both ends and in the middle
static std::vector<uint64_t> deal(uint64_t n, uint32_t m) {
  std::vector<uint64_t> rows{0};
  uint64_t left = n;
  for (uint32_t s = 0; s < m; s++) {
    uint64_t take = left / (m - s) + (s % 2 ? 1 : 0);
    if (take > left || s + 1 == m) take = left;
    rows.push_back(take);
    left -= take;
    if (s == m / 2) rows.push_back(0);
  }
  rows.push_back(0);
  return rows;
}

// source row r -> message: the rows of the sources interleaved (what a split by id gives back), a permutation of 0 .. n-1
static std::vector<int64_t> interleave(const std::vector<uint64_t>& rows, uint64_t n) {
  std::vector<int64_t> idx(n);
  std::vector<uint64_t> first;
  uint64_t at = 0;
  for (uint64_t r : rows) { first.push_back(at); at += r; }
  std::vector<uint64_t> used(rows.size(), 0);
  size_t s = 0;
  for (uint64_t p = 0; p < n; p++) {
    while (used[s % rows.size()] == rows[s % rows.size()]) s++;
    idx[first[s % rows.size()] + used[s % rows.size()]++] = (int64_t)p;
    s++;
  }
  return idx;
}

static void check_joins() {
  size_t cases = 0;
  for (uint32_t kind = 0; kind < FRAME_KINDS; kind++)
    for (uint64_t n : {0ull, 1ull, 63ull, 64ull, 65ull, 255ull, 256ull, 257ull, 1024ull, 1100ull})
      for (uint32_t m : {1u, 3u, 32u})
        for (uint64_t chunks : {1ull, 3ull, 7ull})
          for (int with = 0; with < 2; with++) {
            const std::vector<uint64_t> rows = deal(n, m);
            const std::vector<int64_t> idx = with ? interleave(rows, n) : std::vector<int64_t>();
            const std::string what = std::string(kind ? "single_object" : "confluent") + ", " + std::to_string(m) + " sources" + (with ? ", interleaved" : ", in order");
            const Outcome R = run_join(kind, rows, idx, chunks, what.c_str());
            CHECK(R.ran && R.bad_range == kJoinNone && R.verdict == JOIN_OK, "%s n=%llu: the join did not run", what.c_str(), (unsigned long long)n);
            cases++;
          }
  // more than 256 tiles: the scan's carry crosses its own round
  const uint64_t big = 256ull * 256 + 300;
  for (int with = 0; with < 2; with++) {
    const std::vector<uint64_t> rows = deal(big, 3);
    const Outcome R = run_join(with ? FRAME_SINGLE_OBJECT : FRAME_CONFLUENT, rows, with ? interleave(rows, big) : std::vector<int64_t>(), 3, "257 tiles");
    CHECK(R.ran, "257 tiles: the join did not run");
    cases++;
  }
  std::printf("frame_join_check: %zu join cases\n", cases);
}

static void check_verdicts() {
  size_t cases = 0;
  for (uint64_t n : {65ull, 1100ull}) {
    const std::vector<uint64_t> rows = deal(n, 3);
    const std::vector<int64_t> good = interleave(rows, n);
    const uint64_t last_tile = (join_tiles(n) - 1) * kJoinTile;
    for (int where = 0; where < 2; where++) {
      const uint64_t r = where ? n - 1 : 3;       // a source row of the first / of the last tile
      const uint64_t other = where ? n - 3 : 40;  // another row
      CHECK(r / kJoinTile == (where ? last_tile / kJoinTile : 0), "row %llu is in the wrong tile", (unsigned long long)r);
      // a duplicate: row r names what row `other` names; the position row r had named is now a hole
      {
        std::vector<int64_t> idx = good;
        idx[r] = idx[other];
        const uint64_t twice = (uint64_t)good[other], never = (uint64_t)good[r];
        const Outcome R = run_join(FRAME_CONFLUENT, rows, idx, 3, "a duplicate");
        CHECK(!R.ran && R.bad_range == kJoinNone, "a duplicate at n=%llu: the join ran", (unsigned long long)n);
        CHECK(R.verdict == (never < twice ? JOIN_NEVER : JOIN_TWICE) && R.at == (never < twice ? never : twice), "a duplicate at n=%llu: verdict %u at %llu", (unsigned long long)n,
              (unsigned)R.verdict, (unsigned long long)R.at);
        cases++;
      }
      // a hole below every duplicate, and a duplicate below the hole
      for (int low_hole = 0; low_hole < 2; low_hole++) {
        std::vector<int64_t> idx = good;
        const int64_t lo = where ? (int64_t)n - 2 : 1, hi = where ? (int64_t)n - 1 : 50;      // positions of the first / of the last tile
        uint64_t a = 0, b = 0;      // the rows that name lo and hi
        for (uint64_t q = 0; q < n; q++) { if (good[q] == lo) a = q; if (good[q] == hi) b = q; }
        if (low_hole) idx[a] = hi; else idx[b] = lo;
        const Outcome R = run_join(FRAME_SINGLE_OBJECT, rows, idx, 1, "a hole");
        CHECK(!R.ran && R.verdict == (low_hole ? JOIN_NEVER : JOIN_TWICE) && R.at == (uint64_t)lo, "a hole at n=%llu (%d): verdict %u at %llu", (unsigned long long)n, low_hole,
              (unsigned)R.verdict, (unsigned long long)R.at);
        cases++;
      }
      // out of range: n, -1, and two of them (the lower source row decides, before any duplicate is looked at)
      for (int64_t v : {(int64_t)n, (int64_t)-1}) {
        std::vector<int64_t> idx = good;
        idx[r] = v;
        idx[other] = idx[other == 0 ? 1 : 0];      // (a duplicate as well)
        if (!where) idx[n - 1] = (int64_t)n + 5;
        const Outcome R = run_join(FRAME_CONFLUENT, rows, idx, 2, "out of range");
        CHECK(!R.ran && R.bad_range == r, "out of range at n=%llu: row %llu, expected %llu", (unsigned long long)n, (unsigned long long)R.bad_range, (unsigned long long)r);
        cases++;
      }
    }
  }
  std::printf("frame_join_check: %zu verdict cases\n", cases);
}

int main() {
  check_headers();
  check_copy_plan();
  check_joins();
  check_verdicts();
  std::printf("frame_join_check: %zu checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
