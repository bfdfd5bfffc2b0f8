// Stand-alone check of the container salvage scan (pyruhvro_amd/csrc/container_scan.cpp container_salvage) for sanitizer
// builds: no HIP, no Python.  The twin of container_scan_check.cpp: a valid 3-block container, every prefix of it, every
// single-bit flip of its header and of every block's framing and sync marker, and a hostile 1 MB buffer that is nothing but
// repeated sync markers -- each input in a heap block of exactly its own size, so that a read past `len` is a
// heap-buffer-overflow for AddressSanitizer.  Exit status 0 = every property held.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I pyruhvro_amd/csrc
//       tools/container_salvage_check.cpp pyruhvro_amd/csrc/container_scan.cpp -o container_salvage_check && ./container_salvage_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "container_scan.h"

typedef std::vector<uint8_t> Bytes;

static void put_long(Bytes& o, int64_t v) {
  uint64_t z = ((uint64_t)v << 1) ^ (uint64_t)(v >> 63);
  while (z >= 0x80) { o.push_back((uint8_t)(z | 0x80)); z >>= 7; }
  o.push_back((uint8_t)z);
}
static void put_bytes(Bytes& o, const std::string& s) {
  put_long(o, (int64_t)s.size());
  o.insert(o.end(), s.begin(), s.end());
}

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { failures++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static size_t n_inputs = 0, n_salvaged = 0, n_gaps = 0, n_strict_ok = 0;

// Both scans over exactly these bytes, and every property that holds for any input.  Returns false if the header was refused.
static bool check(const uint8_t* p, size_t n, const char* what, size_t a, int b, rhc::SalvageInfo& sv) {
  std::unique_ptr<uint8_t[]> exact(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(exact.get(), p, n);
  const uint8_t* d = n ? exact.get() : nullptr;
  n_inputs++;
  rhc::ContainerInfo ci;
  const std::string strict = rhc::container_scan(d, n, ci);
  const std::string msg = rhc::container_salvage(d, n, sv);
  if (!msg.empty()) {
    EXPECT(msg == strict, "%s %zu/%d: the salvage scan refuses the header with '%s', the strict scan says '%s'", what, a, b, msg.c_str(), strict.c_str());
    EXPECT(msg.rfind("container: ", 0) == 0 && msg.rfind("container: block ", 0) != 0, "%s %zu/%d: message '%s'", what, a, b, msg.c_str());
    return false;
  }
  n_salvaged++;
  n_gaps += sv.gaps.size();
  const rhc::ContainerInfo& t = sv.info;
  const size_t nb = t.start.size();
  EXPECT(t.end.size() == nb && t.first.size() == nb + 1 && sv.header_offset.size() == nb && sv.count.size() == nb && sv.refused.size() == nb,
         "%s %zu/%d: table sizes", what, a, b);
  // blocks and gaps, merged by offset, tile [header_end, n)
  uint64_t at = sv.header_end;
  size_t ib = 0, ig = 0;
  EXPECT(at <= n, "%s %zu/%d: header end %llu past the input", what, a, b, (unsigned long long)at);
  while (ib < nb || ig < sv.gaps.size()) {
    if (ib < nb && sv.header_offset[ib] == at) {
      EXPECT(t.start[ib] > at && t.start[ib] <= t.end[ib] && t.end[ib] + 16 <= n, "%s %zu/%d: block %zu out of bounds", what, a, b, ib);
      if (!(t.start[ib] > at && t.start[ib] <= t.end[ib] && t.end[ib] + 16 <= n)) return true;
      EXPECT(std::memcmp(d + t.end[ib], t.sync, 16) == 0, "%s %zu/%d: block %zu has no marker", what, a, b, ib);
      EXPECT(t.first[ib + 1] - t.first[ib] == (sv.refused[ib] ? 0 : sv.count[ib]), "%s %zu/%d: block %zu first", what, a, b, ib);
      at = t.end[ib] + 16;
      ib++;
    } else if (ig < sv.gaps.size() && sv.gaps[ig].offset == at) {
      const rhc::SalvageInfo::Gap& g = sv.gaps[ig];
      EXPECT(g.block == ib, "%s %zu/%d: gap %zu names block %llu, %zu are framed", what, a, b, ig, (unsigned long long)g.block, ib);
      EXPECT(g.length > 0 && g.length <= n - at, "%s %zu/%d: gap %zu length", what, a, b, ig);
      if (!(g.length > 0 && g.length <= n - at)) return true;
      EXPECT(g.length >= 16 || at + g.length == n, "%s %zu/%d: gap %zu of %llu bytes does not end the scan", what, a, b, ig, (unsigned long long)g.length);
      if (at + g.length < n) EXPECT(std::memcmp(d + at + g.length - 16, t.sync, 16) == 0, "%s %zu/%d: gap %zu does not end behind a marker", what, a, b, ig);
      EXPECT(g.message.rfind("container: block " + std::to_string(ib) + ": ", 0) == 0, "%s %zu/%d: gap message '%s'", what, a, b, g.message.c_str());
      at += g.length;
      ig++;
    } else {
      EXPECT(false, "%s %zu/%d: nothing starts at byte %llu", what, a, b, (unsigned long long)at);
      return true;
    }
  }
  EXPECT(at == n, "%s %zu/%d: the tiling ends at %llu of %zu", what, a, b, (unsigned long long)at, n);
  EXPECT(sv.steps <= 2 * (uint64_t)n + 2, "%s %zu/%d: %llu steps for %zu bytes", what, a, b, (unsigned long long)sv.steps, n);
  if (strict.empty()) {
    n_strict_ok++;
    EXPECT(sv.gaps.empty() && t.start == ci.start && t.end == ci.end && t.first == ci.first, "%s %zu/%d: differs from the strict scan's table", what, a, b);
    for (size_t i = 0; i < nb; i++) EXPECT(!sv.refused[i], "%s %zu/%d: block %zu refused", what, a, b, i);
    EXPECT(t.schema == ci.schema && t.codec == ci.codec && std::memcmp(t.sync, ci.sync, 16) == 0 && t.metadata == ci.metadata, "%s %zu/%d: header fields", what, a, b);
  } else {
    // the strict message is the first thing the salvage scan reports: its first gap, or its first refused count
    std::string first_msg;
    uint64_t first_at = ~0ull;
    if (!sv.gaps.empty()) { first_msg = sv.gaps[0].message; first_at = sv.gaps[0].offset; }
    for (size_t i = 0; i < nb; i++)
      if (sv.refused[i] && sv.header_offset[i] < first_at) { first_msg = "container: block " + std::to_string(i) + ": record count out of range"; first_at = sv.header_offset[i]; break; }
    EXPECT(first_msg == strict, "%s %zu/%d: the first report is '%s', the strict scan says '%s'", what, a, b, first_msg.c_str(), strict.c_str());
  }
  return true;
}

int main() {
  const std::string schema = "{\"type\":\"record\",\"name\":\"R\",\"fields\":[{\"name\":\"a\",\"type\":\"long\"}]}";
  uint8_t sync[16];
  for (int i = 0; i < 16; i++) sync[i] = (uint8_t)(0xA0 + i);

  Bytes f = {'O', 'b', 'j', 1};
  put_long(f, 2);
  put_bytes(f, "avro.schema"); put_bytes(f, schema);
  put_bytes(f, "avro.codec"); put_bytes(f, "null");
  put_long(f, 0);
  f.insert(f.end(), sync, sync + 16);
  const size_t hdr = f.size();
  const size_t counts[3] = {3, 0, 200}, sizes[3] = {5, 0, 300};
  std::vector<size_t> framing_at, framing_len, block_end;
  for (int b = 0; b < 3; b++) {
    const size_t at = f.size();
    put_long(f, (int64_t)counts[b]);
    put_long(f, (int64_t)sizes[b]);
    framing_at.push_back(at);
    framing_len.push_back(f.size() - at);
    for (size_t i = 0; i < sizes[b]; i++) f.push_back((uint8_t)(i * 7 + b));
    f.insert(f.end(), sync, sync + 16);
    block_end.push_back(f.size());
  }

  rhc::SalvageInfo sv;
  EXPECT(check(f.data(), f.size(), "valid", 0, 0, sv) && sv.gaps.empty() && sv.info.nb() == 3 && sv.info.n() == 203, "the valid file");
  EXPECT(sv.header_end == hdr && sv.header_offset.size() == 3 && sv.header_offset[0] == hdr && sv.header_offset[1] == block_end[0] && sv.header_offset[2] == block_end[1], "header offsets");

  // every prefix: a cut behind the header leaves the whole blocks in front of it and one gap to the end
  for (size_t cut = 0; cut < f.size(); cut++) {
    const bool ok = check(f.data(), cut, "prefix", cut, 0, sv);
    EXPECT(ok == (cut >= hdr), "prefix of %zu bytes: header %s", cut, ok ? "accepted" : "refused");
    if (!ok) continue;
    const size_t whole = (cut >= block_end[0]) + (cut >= block_end[1]);
    const size_t done = whole == 0 ? hdr : block_end[whole - 1];
    EXPECT(sv.info.nb() == whole, "prefix of %zu bytes: %llu blocks, not %zu", cut, (unsigned long long)sv.info.nb(), whole);
    EXPECT(sv.gaps.size() == (cut > done ? 1u : 0u), "prefix of %zu bytes: %zu gaps", cut, sv.gaps.size());
    if (cut > done && sv.gaps.size() == 1) EXPECT(sv.gaps[0].offset == done && sv.gaps[0].length == cut - done, "prefix of %zu bytes: the gap", cut);
  }

  // every single-bit flip of the header, of the blocks' framing and of their markers
  size_t flips = 0;
  Bytes g = f;
  auto flip_range = [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++)
      for (int bit = 0; bit < 8; bit++, flips++) {
        g[i] ^= (uint8_t)(1u << bit);
        check(g.data(), g.size(), "flip", i, bit, sv);
        g[i] ^= (uint8_t)(1u << bit);
      }
  };
  flip_range(0, hdr);
  for (int b = 0; b < 3; b++) {
    flip_range(framing_at[b], framing_at[b] + framing_len[b]);
    flip_range(block_end[b] - 16, block_end[b]);
  }
  // a flipped marker byte of block 0: one gap that swallows block 0 and block 1, then block 2 is framed
  g = f;
  g[block_end[0] - 1] ^= 1;
  EXPECT(check(g.data(), g.size(), "marker", 0, 0, sv) && sv.gaps.size() == 1 && sv.info.nb() == 1, "flipped marker: %zu gaps, %llu blocks", sv.gaps.size(), (unsigned long long)sv.info.nb());
  if (sv.gaps.size() == 1) EXPECT(sv.gaps[0].offset == hdr && sv.gaps[0].length == block_end[1] - hdr && sv.gaps[0].message == "container: block 0: sync marker mismatch", "flipped marker: the gap");
  // the same flips in a file cut in the middle of its last block
  g.assign(f.begin(), f.begin() + (long)(block_end[1] + 40));
  flip_range(hdr, hdr + framing_len[0]);
  // a count that the running total cannot take: the block is framed and refused
  {
    Bytes x(f.begin(), f.begin() + (long)hdr);
    put_long(x, (int64_t)((1ull << 62) + 1)); put_long(x, 2); x.push_back(1); x.push_back(2);
    x.insert(x.end(), sync, sync + 16);
    x.insert(x.end(), f.begin() + (long)hdr, f.end());
    EXPECT(check(x.data(), x.size(), "range", 0, 0, sv) && sv.info.nb() == 4 && sv.refused[0] == 1 && sv.gaps.empty() && sv.info.n() == 203, "count out of range");
  }

  // hostile: 1 MB of nothing but sync markers behind the header -- every marker is a 16-byte gap; the work stays linear
  {
    const size_t total = 1 << 20;
    Bytes x(f.begin(), f.begin() + (long)hdr);
    while (x.size() + 16 <= total) x.insert(x.end(), sync, sync + 16);
    EXPECT(check(x.data(), x.size(), "markers", 0, 0, sv), "the hostile buffer's header");
    EXPECT(sv.info.nb() == 0 && sv.gaps.size() == (x.size() - hdr) / 16, "hostile buffer: %llu blocks, %zu gaps", (unsigned long long)sv.info.nb(), sv.gaps.size());
    EXPECT(sv.steps <= 2 * ((x.size() - hdr) / 16) + 2, "hostile buffer: %llu steps for %zu markers", (unsigned long long)sv.steps, (x.size() - hdr) / 16);
    std::printf("hostile buffer of sync markers: %zu bytes, %zu gaps, %llu loop turns\n", x.size(), sv.gaps.size(), (unsigned long long)sv.steps);
    // ... and of the marker's first byte alone: every position starts a compare, none matches
    Bytes y(f.begin(), f.begin() + (long)hdr);
    y.resize(total, sync[0]);
    EXPECT(check(y.data(), y.size(), "first bytes", 0, 0, sv) && sv.info.nb() == 0 && sv.gaps.size() == 1, "buffer of first bytes");
    EXPECT(sv.steps <= y.size() + 2, "buffer of first bytes: %llu steps for %zu bytes", (unsigned long long)sv.steps, y.size());
    std::printf("hostile buffer of the marker's first byte: %zu bytes, %zu gaps, %llu loop turns\n", y.size(), sv.gaps.size(), (unsigned long long)sv.steps);
  }

  std::printf("container_salvage_check: %zu inputs (%zu salvaged, %zu accepted by the strict scan too), %zu bit flips, %zu gaps, %d failures\n",
              n_inputs, n_salvaged, n_strict_ok, flips, n_gaps, failures);
  return failures ? 1 : 0;
}
