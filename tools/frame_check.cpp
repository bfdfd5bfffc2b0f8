// CPU check of pyruhvro_amd/csrc/frame_core.h (the twin of filter_check.cpp: its own main, no HIP, no Python).
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I pyruhvro_amd/csrc
//       tools/frame_check.cpp -o frame_check && ./frame_check
//
// 1. frame_id / frame_class / frame_verdict against a plain restatement (shifts written out per framing, a linear search), over the
//    id edges: confluent 0, 1, 0x01000000, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF; single-object values that differ only in the
//    lowest or only in the highest byte; lists of 1, 2, 3 and 32 ids; messages of every length from 0 to the header and beyond.
// 2. The split as the kernels run it (frame.hip: classify with its tile histogram, scan, offsets, gather in 16-lane groups) against
//    std::vector loops in the manner of std::stable_partition, for n in {0, 1, 63, 64, 65, 255, 256, 257, 1024, 1100}, m in
//    {1, 2, 3, 32}, both framings, the class patterns named below.  Every buffer sits in a heap block of exactly its size.
// Exit status 0 = no failure; the last line says what ran.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "frame_core.h"

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
static std::vector<uint8_t> make_message(uint32_t kind, uint64_t id, const std::vector<uint8_t>& payload) {
  std::vector<uint8_t> m;
  if (kind == FRAME_CONFLUENT) {
    m = {0x00, (uint8_t)(id >> 24), (uint8_t)(id >> 16), (uint8_t)(id >> 8), (uint8_t)id};
  } else {
    m = {0xC3, 0x01};
    for (int i = 0; i < 8; i++) m.push_back((uint8_t)(id >> (8 * i)));
  }
  m.insert(m.end(), payload.begin(), payload.end());
  return m;
}

enum RefVerdict { REF_UNKNOWN = -1, REF_SHORT = -2, REF_MARKER = -3 };
static int ref_verdict(uint32_t kind, const std::vector<uint8_t>& msg, const std::vector<uint64_t>& ids) {
  uint64_t id = 0;
  if (kind == FRAME_CONFLUENT) {
    if (msg.size() < 5) return REF_SHORT;
    if (msg[0] != 0x00) return REF_MARKER;
    id = ((uint64_t)msg[1] << 24) | ((uint64_t)msg[2] << 16) | ((uint64_t)msg[3] << 8) | (uint64_t)msg[4];
  } else {
    if (msg.size() < 10) return REF_SHORT;
    if (msg[0] != 0xC3 || msg[1] != 0x01) return REF_MARKER;
    for (int i = 7; i >= 0; i--) id = (id << 8) | msg[2 + i];
  }
  for (size_t c = 0; c < ids.size(); c++)
    if (ids[c] == id) return (int)c;
  return REF_UNKNOWN;
}
static int as_ref(uint8_t v) { return v == kFrameShort ? REF_SHORT : v == kFrameBadMarker ? REF_MARKER : v == kFrameUnknown ? REF_UNKNOWN : (int)v; }

// ids of a call: ascending, distinct, with the edges of the framing among them
static std::vector<uint64_t> id_list(uint32_t kind, uint32_t m) {
  static const uint64_t kConfluent[] = {0, 1, 0x01000000ull, 0x7FFFFFFFull, 0x80000000ull, 0xFFFFFFFFull};
  // single-object: values that differ only in the lowest byte, only in the highest byte
  static const uint64_t kSingle[] = {0x1122334455667700ull, 0x1122334455667701ull, 0x9122334455667700ull, 0, 0x8000000000000000ull, ~0ull};
  std::vector<uint64_t> v;
  const uint64_t* edges = kind == FRAME_CONFLUENT ? kConfluent : kSingle;
  for (uint32_t i = 0; i < 6 && v.size() < m; i++) v.push_back(edges[i]);
  uint64_t x = kind == FRAME_CONFLUENT ? 1000 : 0x0100000000000000ull;
  while (v.size() < m) { v.push_back(x); x += kind == FRAME_CONFLUENT ? 7 : 0x0100000000000007ull; }
  for (size_t i = 1; i < v.size(); i++)      // insertion sort
    for (size_t j = i; j > 0 && v[j] < v[j - 1]; j--) { const uint64_t t = v[j]; v[j] = v[j - 1]; v[j - 1] = t; }
  return v;
}
static uint64_t unknown_id(uint32_t kind, uint32_t salt) {      // in no list of id_list
  return kind == FRAME_CONFLUENT ? 0x00000100ull + (salt % 3) * 0x00010000ull : 0x1122334455667702ull + (uint64_t)(salt % 3) * 0x0100000000000000ull;
}

static void check_headers() {
  for (uint32_t kind = 0; kind < FRAME_KINDS; kind++) {
    const FrameDesc d = frame_desc(kind);
    CHECK(d.header == d.marker_len + d.id_len && d.header <= kFrameMaxHeader, "header layout of framing %u", kind);
    for (uint32_t m : {1u, 2u, 3u, 6u, 32u}) {
      const std::vector<uint64_t> ids = id_list(kind, m);
      for (size_t c = 1; c < ids.size(); c++) CHECK(ids[c - 1] < ids[c], "the id list is ascending");
      std::unique_ptr<uint64_t[]> idb(new uint64_t[m]);
      std::memcpy(idb.get(), ids.data(), 8 * m);
      std::vector<uint64_t> probe = ids;
      for (uint32_t s = 0; s < 3; s++) probe.push_back(unknown_id(kind, s));
      for (uint64_t id : ids) { probe.push_back(id + 1); probe.push_back(id - 1); }
      for (uint64_t id : probe) {
        if (kind == FRAME_CONFLUENT) id &= 0xFFFFFFFFull;
        for (size_t plen : {0u, 1u, 17u}) {
          const std::vector<uint8_t> msg = make_message(kind, id, std::vector<uint8_t>(plen, 0xAB));
          // every prefix of the message, a wrong marker byte in either place: exact heap blocks
          for (size_t len = 0; len <= msg.size(); len++) {
            if (len > d.header && len < msg.size()) continue;
            std::unique_ptr<uint8_t[]> blk(new uint8_t[len]);
            if (len) std::memcpy(blk.get(), msg.data(), len);
            const std::vector<uint8_t> part(msg.begin(), msg.begin() + (long)len);
            const uint8_t v = frame_verdict(blk.get(), 0, len, d, idb.get(), m);
            CHECK(as_ref(v) == ref_verdict(kind, part, ids), "framing %u m=%u id=%llx len=%zu: verdict %d", kind, m, (unsigned long long)id, len, (int)v);
            if (len >= d.header) {
              CHECK(frame_id(blk.get(), d) == id, "framing %u: id %llx read as %llx", kind, (unsigned long long)id, (unsigned long long)frame_id(blk.get(), d));
              for (uint32_t k = 0; k < d.marker_len; k++) {
                blk[k] ^= 0x40;
                std::vector<uint8_t> bad = part;
                bad[k] ^= 0x40;
                CHECK(frame_verdict(blk.get(), 0, len, d, idb.get(), m) == kFrameBadMarker && ref_verdict(kind, bad, ids) == REF_MARKER, "framing %u: marker byte %u", kind, k);
                blk[k] ^= 0x40;
              }
            }
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// the split: the kernels' steps in the kernels' order, on exact heap blocks
// ---------------------------------------------------------------------------
// what message i is: a class, -1 = an unknown id, -2 = too short, -3 = a wrong marker
typedef int (*Pattern)(uint64_t i, uint64_t n, uint32_t m);
static int pat_one(uint64_t, uint64_t, uint32_t m) { return (int)(m - 1); }
static int pat_alternating(uint64_t i, uint64_t, uint32_t m) { return (int)(i % m); }
static int pat_wave_runs(uint64_t i, uint64_t, uint32_t m) { return (int)((i / 64) % m); }      // runs that end on wavefront edges
static int pat_tile_runs(uint64_t i, uint64_t, uint32_t m) { return (int)((i / 256) % m); }     // ... on tile edges
static int pat_last_only(uint64_t i, uint64_t n, uint32_t m) { return i + 1 == n ? (int)(m - 1) : 0; }      // a class seen only in the last message
static int pat_never(uint64_t i, uint64_t, uint32_t m) { return m > 1 ? (int)(i % (m - 1)) : 0; }           // class m - 1 never seen
static int pat_unknowns(uint64_t i, uint64_t, uint32_t m) { return i % 7 == 3 ? -1 : (int)((i * 5) % m); }  // unknown ids sprinkled in
static int pat_bad(uint64_t i, uint64_t n, uint32_t m) {                                                    // ... and bad frames
  if (i == n / 2) return -2;
  if (i == n - 1 && n > 2) return -3;
  return i % 11 == 5 ? -1 : (int)((i * 3) % m);
}
static int pat_random(uint64_t i, uint64_t, uint32_t m) {
  uint64_t x = 88172645463325252ull + i * 0x9E3779B97F4A7C15ull;
  x ^= x << 13; x ^= x >> 7; x ^= x << 17;
  return (int)((x >> 20) % (m + 1)) - 1;
}

static size_t payload_len(uint64_t i) {      // 0 (the bare header), 1, 15, 16, 17, 31, 33 and a few long ones among them
  static const size_t kLens[] = {0, 1, 15, 16, 17, 31, 33, 2, 7, 40};
  return i % 37 == 9 ? 64 + i % 90 : i % 101 == 50 ? 700 : kLens[i % 10];
}

static void check_split(uint32_t kind, uint64_t n, uint32_t m, Pattern pat, const char* what, bool skip_unknown) {
  const FrameDesc d = frame_desc(kind);
  const std::vector<uint64_t> ids = id_list(kind, m);
  // ---- the input, packed as the engine packs it, and the plain restatement beside it
  std::vector<std::vector<uint8_t>> msgs;
  std::vector<int> want;
  for (uint64_t i = 0; i < n; i++) {
    const int w = pat(i, n, m);
    std::vector<uint8_t> payload(payload_len(i));
    for (size_t b = 0; b < payload.size(); b++) payload[b] = (uint8_t)(i * 131 + b * 17 + 1);
    std::vector<uint8_t> msg = make_message(kind, w >= 0 ? ids[(size_t)w] : unknown_id(kind, (uint32_t)i), payload);
    if (w == -2) msg.resize(i % d.header);      // 0 .. header - 1 bytes
    if (w == -3) msg[i % d.marker_len] ^= 0x21;
    msgs.push_back(msg);
    want.push_back(w);
  }
  std::unique_ptr<uint64_t[]> off(new uint64_t[n + 1]);
  off[0] = 0;
  for (uint64_t i = 0; i < n; i++) off[i + 1] = off[i] + msgs[i].size();
  const uint64_t data_len = off[n];
  std::unique_ptr<uint8_t[]> data(new uint8_t[data_len]);
  for (uint64_t i = 0; i < n; i++)
    if (!msgs[i].empty()) std::memcpy(data.get() + off[i], msgs[i].data(), msgs[i].size());
  std::vector<std::vector<int64_t>> exp_idx(m + 1);
  std::vector<std::vector<uint64_t>> exp_off(m, std::vector<uint64_t>{0});
  std::vector<std::vector<uint8_t>> exp_data(m);
  uint64_t exp_bad = kFrameNoFailure;
  for (uint64_t i = 0; i < n; i++) {
    const int r = ref_verdict(kind, msgs[i], ids);
    CHECK(r == want[i], "%s: the generator made message %llu a %d, not a %d", what, (unsigned long long)i, r, want[i]);
    const bool fails = r == REF_SHORT || r == REF_MARKER || (r == REF_UNKNOWN && !skip_unknown);
    if (fails && exp_bad == kFrameNoFailure) exp_bad = i;
    if (r == REF_UNKNOWN) exp_idx[m].push_back((int64_t)i);
    if (r >= 0) {
      exp_idx[(size_t)r].push_back((int64_t)i);
      exp_data[(size_t)r].insert(exp_data[(size_t)r].end(), msgs[i].begin() + d.header, msgs[i].end());
      exp_off[(size_t)r].push_back(exp_data[(size_t)r].size());
    }
  }
  std::unique_ptr<uint64_t[]> idb(new uint64_t[m]);
  std::memcpy(idb.get(), ids.data(), 8 * m);

  // ---- rh_k_frame_classify: verdicts, the tile histogram, the lowest failing index
  const uint64_t ntiles = frame_tiles(n);
  const uint64_t cells = (uint64_t)(m + 1) * ntiles;
  std::unique_ptr<uint8_t[]> cls(new uint8_t[n]);
  std::unique_ptr<uint64_t[]> tile_cnt(new uint64_t[cells]), tile_bytes(new uint64_t[cells]), pre_cnt(new uint64_t[cells]), pre_bytes(new uint64_t[cells]);
  uint64_t first_bad = kFrameNoFailure;
  for (uint64_t tile = 0; tile < ntiles; tile++) {
    uint64_t h_cnt[kMaxFrameIds + 1] = {0}, h_bytes[kMaxFrameIds + 1] = {0};
    for (uint32_t t = 0; t < kFrameTile; t++) {
      const uint64_t i = tile * kFrameTile + t;
      if (i >= n) continue;
      const uint64_t b = off[i], e = off[i + 1];
      const uint8_t v = (b <= e && e <= data_len) ? frame_verdict(data.get(), b, e, d, idb.get(), m) : kFrameShort;
      cls[i] = v;
      const uint32_t bin = frame_bin(v, m);
      if (bin > m || (bin == m && !skip_unknown)) {
        if (i < first_bad) first_bad = i;
      } else {
        h_cnt[bin]++;
        h_bytes[bin] += frame_payload_len(b, e, bin, m, d);
      }
    }
    for (uint32_t c = 0; c <= m; c++) {
      tile_cnt[frame_table_at(ntiles, c, tile)] = h_cnt[c];
      tile_bytes[frame_table_at(ntiles, c, tile)] = h_bytes[c];
    }
  }
  CHECK(first_bad == exp_bad, "%s n=%llu m=%u: lowest failure %llu, expected %llu", what, (unsigned long long)n, m, (unsigned long long)first_bad,
        (unsigned long long)exp_bad);
  for (uint64_t i = 0; i < n; i++) CHECK(as_ref(cls[i]) == want[i], "%s n=%llu m=%u: verdict of message %llu", what, (unsigned long long)n, m, (unsigned long long)i);
  if (first_bad != kFrameNoFailure) return;      // the call ends here with the failure's message

  // ---- rh_k_frame_scan: one (bin, table) at a time, 256 tiles a round with a carry
  std::unique_ptr<uint64_t[]> totals(new uint64_t[2 * (m + 1)]);
  for (uint32_t blk = 0; blk < 2 * (m + 1); blk++) {
    const uint32_t bin = blk >> 1, which = blk & 1;
    const uint64_t* in = (which ? tile_bytes.get() : tile_cnt.get()) + frame_table_at(ntiles, bin, 0);
    uint64_t* out = (which ? pre_bytes.get() : pre_cnt.get()) + frame_table_at(ntiles, bin, 0);
    uint64_t carry = 0;
    for (uint64_t base = 0; base < ntiles; base += kFrameTile) {
      uint64_t run = 0;
      for (uint32_t t = 0; t < kFrameTile; t++) {
        const uint64_t x = base + t;
        const uint64_t v = x < ntiles ? in[x] : 0;
        if (x < ntiles) out[x] = carry + run;
        run += v;
      }
      carry += run;
    }
    totals[which * (m + 1) + bin] = carry;
  }
  uint64_t seen = 0;
  std::vector<uint64_t> index_base(m + 1);
  for (uint32_t c = 0; c <= m; c++) {
    CHECK(totals[c] == exp_idx[c].size(), "%s n=%llu m=%u: class %u has %llu messages, expected %zu", what, (unsigned long long)n, m, c,
          (unsigned long long)totals[c], exp_idx[c].size());
    if (c < m) CHECK(totals[m + 1 + c] == exp_data[c].size(), "%s n=%llu m=%u: class %u has %llu payload bytes, expected %zu", what, (unsigned long long)n, m, c,
                     (unsigned long long)totals[m + 1 + c], exp_data[c].size());
    index_base[c] = seen;
    seen += totals[c];
  }
  CHECK(totals[m + 1 + m] == 0, "the unknown ids have no payload");
  CHECK(seen == n, "%s n=%llu m=%u: the bins hold %llu messages", what, (unsigned long long)n, m, (unsigned long long)seen);
  if (seen != n) return;

  // ---- the leases: one per class for payload and offsets, exactly sized
  std::unique_ptr<int64_t[]> indices(new int64_t[n]);
  std::unique_ptr<uint64_t[]> dst(new uint64_t[n]);
  std::vector<std::unique_ptr<uint64_t[]>> noff(m);
  std::vector<std::unique_ptr<uint8_t[]>> out(m);
  for (uint64_t i = 0; i < n; i++) { indices[i] = -1; dst[i] = ~0ull; }
  for (uint32_t c = 0; c < m; c++) {
    noff[c].reset(new uint64_t[totals[c] + 1]);
    for (uint64_t r = 0; r <= totals[c]; r++) noff[c][r] = ~0ull;
    out[c].reset(new uint8_t[totals[m + 1 + c]]);
    std::memset(out[c].get(), 0, totals[m + 1 + c]);
  }
  // ---- rh_k_frame_offsets: per tile, per bin the table says is present
  for (uint64_t tile = 0; tile < ntiles; tile++) {
    for (uint32_t c = 0; c <= m; c++) {
      const uint64_t at = frame_table_at(ntiles, c, tile);
      if (tile_cnt[at] == 0) continue;
      uint64_t r = 0, q = 0;
      for (uint32_t t = 0; t < kFrameTile; t++) {
        const uint64_t i = tile * kFrameTile + t;
        if (i >= n || frame_bin(cls[i], m) != c) continue;
        const uint64_t len = frame_payload_len(off[i], off[i + 1], c, m, d);
        const uint64_t rank = frame_rank(pre_cnt[at], r), byte = frame_byte(pre_bytes[at], q);
        if (index_base[c] + rank < n) indices[index_base[c] + rank] = (int64_t)i;
        else CHECK(false, "%s: an index past the list", what);
        if (c < m) {
          if (rank < totals[c]) noff[c][rank] = byte;
          else CHECK(false, "%s: an offset past the class's list", what);
          dst[i] = byte;
        }
        r++;
        q += len;
      }
      CHECK(r == tile_cnt[at] && q == tile_bytes[at], "%s: tile %llu, bin %u: the offsets pass saw other messages than classify", what, (unsigned long long)tile, c);
    }
  }
  if (ntiles)
    for (uint32_t c = 0; c < m; c++) noff[c][totals[c]] = totals[m + 1 + c];
  else
    for (uint32_t c = 0; c < m; c++) noff[c][0] = 0;      // (no launch: the engine zeroes the one entry)
  // ---- rh_k_frame_gather: a wavefront per 64 messages, 16 rounds of four 16-lane groups
  uint64_t copied = 0;
  for (uint64_t r0 = 0; r0 < n; r0 += 64) {
    for (uint32_t k = 0; k < kFrameRounds; k++)
      for (uint32_t group = 0; group < kFrameGroups; group++) {
        const uint64_t i = r0 + kFrameGroups * k + group;
        if (i >= n || cls[i] >= m) continue;
        const uint32_t c = cls[i];
        const uint64_t b = off[i], len = (off[i + 1] - b) - d.header;
        if (!len) continue;
        if (dst[i] + len > totals[m + 1 + c]) { CHECK(false, "%s: a payload would be copied past its region", what); continue; }
        const uint8_t* s = data.get() + b + d.header;
        uint8_t* o = out[c].get() + dst[i];
        // (the region's start stands for a 16-byte aligned address, as a lease's is)
        const FrameCopy p = frame_copy_plan(dst[i], len);
        CHECK(p.head + 16 * p.nvec + p.tail == len && p.head < 16 && p.tail < 16 && (p.nvec == 0 || (dst[i] + p.head) % 16 == 0), "%s: copy plan of %llu bytes at %llu", what,
              (unsigned long long)len, (unsigned long long)dst[i]);
        for (uint32_t sub = 0; sub < kFrameGroup; sub++) {
          if (sub < p.head) o[sub] = s[sub];
          for (uint64_t v = sub; v < p.nvec; v += kFrameGroup) std::memcpy(o + p.head + (v << 4), s + p.head + (v << 4), 16);
          const uint64_t done = p.head + (p.nvec << 4);
          if (sub < p.tail) o[done + sub] = s[done + sub];
        }
        copied += len;
      }
  }
  // ---- against the plain restatement
  uint64_t exp_bytes = 0;
  for (uint32_t c = 0; c <= m; c++)
    for (size_t r = 0; r < exp_idx[c].size(); r++)
      CHECK(indices[index_base[c] + r] == exp_idx[c][r], "%s n=%llu m=%u: index %zu of class %u is %lld, expected %lld", what, (unsigned long long)n, m, r, c,
            (long long)indices[index_base[c] + r], (long long)exp_idx[c][r]);
  for (uint32_t c = 0; c < m; c++) {
    for (size_t r = 0; r < exp_off[c].size(); r++)
      CHECK(noff[c][r] == exp_off[c][r], "%s n=%llu m=%u: offset %zu of class %u is %llu, expected %llu", what, (unsigned long long)n, m, r, c,
            (unsigned long long)noff[c][r], (unsigned long long)exp_off[c][r]);
    CHECK(exp_data[c].empty() || std::memcmp(out[c].get(), exp_data[c].data(), exp_data[c].size()) == 0, "%s n=%llu m=%u: the payloads of class %u differ", what,
          (unsigned long long)n, m, c);
    exp_bytes += exp_data[c].size();
  }
  CHECK(copied == exp_bytes, "%s n=%llu m=%u: %llu bytes copied, expected %llu", what, (unsigned long long)n, m, (unsigned long long)copied, (unsigned long long)exp_bytes);
}

static void check_splits() {
  static const struct { Pattern f; const char* name; bool bad; } kPatterns[] = {
    {pat_one, "all one class", false}, {pat_alternating, "alternating classes", false}, {pat_wave_runs, "runs ending on wavefront edges", false},
    {pat_tile_runs, "runs ending on tile edges", false}, {pat_last_only, "a class seen only in the last message", false},
    {pat_never, "a class never seen", false}, {pat_unknowns, "unknown ids sprinkled in", false}, {pat_bad, "unknowns and bad frames sprinkled in", true},
    {pat_random, "random", false}};
  size_t cases = 0;
  for (uint32_t kind = 0; kind < FRAME_KINDS; kind++)
    for (uint64_t n : {0ull, 1ull, 63ull, 64ull, 65ull, 255ull, 256ull, 257ull, 1024ull, 1100ull})
      for (uint32_t m : {1u, 2u, 3u, 32u})
        for (const auto& p : kPatterns)
          for (int skip = 0; skip < 2; skip++) {
            const std::string what = std::string(kind ? "single_object, " : "confluent, ") + p.name + (skip ? ", unknown ids skipped" : "");
            check_split(kind, n, m, p.f, what.c_str(), skip != 0);
            cases++;
          }
  // more than 256 tiles: the scan's carry crosses its own round
  check_split(FRAME_CONFLUENT, 256ull * 256 + 300, 3, pat_random, "confluent, random, 257 tiles", true);
  check_split(FRAME_SINGLE_OBJECT, 256ull * 256 + 300, 3, pat_alternating, "single_object, alternating, 257 tiles", false);
  cases += 2;
  std::printf("frame_check: %zu split cases\n", cases);
}

int main() {
  check_headers();
  check_splits();
  std::printf("frame_check: %zu checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
