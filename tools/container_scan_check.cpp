// Stand-alone check of the container framing scan (pyruhvro_amd/csrc/container_scan.cpp) for sanitizer builds: no HIP, no
// Python.  Builds a valid 3-block container, then runs the scanner over every prefix of it and over every single-bit flip
// of its header and of every block's framing -- each input in a heap block of exactly its own size, so that a read past
// `len` is a heap-buffer-overflow for AddressSanitizer.  Exit status 0 = every verdict was the expected one.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I pyruhvro_amd/csrc
//       tools/container_scan_check.cpp pyruhvro_amd/csrc/container_scan.cpp -o container_scan_check && ./container_scan_check
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

// the scan of exactly these bytes
static std::string scan(const uint8_t* p, size_t n, rhc::ContainerInfo& ci) {
  std::unique_ptr<uint8_t[]> exact(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(exact.get(), p, n);
  return rhc::container_scan(n ? exact.get() : nullptr, n, ci);
}

int main() {
  const std::string schema = "{\"type\":\"record\",\"name\":\"R\",\"fields\":[{\"name\":\"a\",\"type\":\"long\"}]}";
  uint8_t sync[16];
  for (int i = 0; i < 16; i++) sync[i] = (uint8_t)(0xA0 + i);

  // header: the metadata map in two blocks, the second with a negative count and a byte size
  Bytes f = {'O', 'b', 'j', 1};
  put_long(f, 2);
  put_bytes(f, "avro.schema"); put_bytes(f, schema);
  put_bytes(f, "avro.codec"); put_bytes(f, "null");
  Bytes second;
  put_bytes(second, "who"); put_bytes(second, std::string("t\0st", 4));
  put_long(f, -1); put_long(f, (int64_t)second.size());
  f.insert(f.end(), second.begin(), second.end());
  put_long(f, 0);
  f.insert(f.end(), sync, sync + 16);
  const size_t hdr = f.size();
  // blocks of 3, 0 and 200 records (a 2-byte count; the third size is a 2-byte varint too)
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

  rhc::ContainerInfo ci;
  std::string msg = scan(f.data(), f.size(), ci);
  EXPECT(msg.empty(), "the valid file is refused: %s", msg.c_str());
  EXPECT(ci.schema == schema && ci.codec == "null" && std::memcmp(ci.sync, sync, 16) == 0, "header fields");
  EXPECT(ci.metadata.size() == 1 && ci.metadata[0].first == "who" && ci.metadata[0].second == std::string("t\0st", 4), "metadata");
  EXPECT(ci.nb() == 3 && ci.n() == 203 && ci.first.size() == 4 && ci.first[1] == 3 && ci.first[2] == 3, "block table");
  for (int b = 0; b < 3 && ci.nb() == 3; b++)
    EXPECT(ci.start[b] == framing_at[b] + framing_len[b] && ci.end[b] == ci.start[b] + sizes[b], "block %d bounds", b);

  // every prefix: accepted exactly at the end of the header and at the end of every block
  size_t cuts = 0, refused = 0;
  for (size_t cut = 0; cut < f.size(); cut++, cuts++) {
    msg = scan(f.data(), cut, ci);
    const bool boundary = cut == hdr || cut == block_end[0] || cut == block_end[1];
    EXPECT(msg.empty() == boundary, "prefix of %zu bytes: %s", cut, msg.empty() ? "accepted" : msg.c_str());
    if (!msg.empty()) {
      refused++;
      EXPECT(msg.rfind("container: ", 0) == 0, "prefix of %zu bytes: message '%s'", cut, msg.c_str());
      if (cut > hdr) EXPECT(msg.rfind("container: block ", 0) == 0, "prefix of %zu bytes names no block: '%s'", cut, msg.c_str());
    }
  }

  // every single-bit flip of the header and of the blocks' framing and sync markers: any verdict, no bad read; a message
  // always starts with "container: "
  size_t flips = 0, flip_refused = 0;
  Bytes g = f;
  auto flip_range = [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++)
      for (int bit = 0; bit < 8; bit++, flips++) {
        g[i] ^= (uint8_t)(1u << bit);
        msg = scan(g.data(), g.size(), ci);
        if (!msg.empty()) {
          flip_refused++;
          EXPECT(msg.rfind("container: ", 0) == 0, "flip of byte %zu bit %d: message '%s'", i, bit, msg.c_str());
        } else {
          for (size_t b = 0; b < ci.nb(); b++) EXPECT(ci.start[b] <= ci.end[b] && ci.end[b] <= g.size(), "flip of byte %zu bit %d: block %zu out of bounds", i, bit, b);
        }
        g[i] ^= (uint8_t)(1u << bit);
      }
  };
  flip_range(0, hdr);
  for (int b = 0; b < 3; b++) {
    flip_range(framing_at[b], framing_at[b] + framing_len[b]);
    flip_range(block_end[b] - 16, block_end[b]);
  }
  // ... and the same flips in a file cut in the middle of its last block
  g.assign(f.begin(), f.begin() + (long)(block_end[1] + 40));
  flip_range(0, hdr);

  // hostile lengths
  const int64_t huge[] = {INT64_MAX, INT64_MIN, (int64_t)1 << 62, -((int64_t)1 << 40), (int64_t)f.size(), -1};
  size_t hostile = 0;
  for (int64_t h : huge) {
    for (int where = 0; where < 4; where++, hostile++) {
      Bytes x(f.begin(), f.begin() + (where < 2 ? 4 : (long)hdr));
      if (where == 0) put_long(x, h);                                   // the map's entry count
      if (where == 1) { put_long(x, 1); put_long(x, h); }               // a key length
      if (where == 2) { put_long(x, h); put_long(x, 5); }               // a block's record count
      if (where == 3) { put_long(x, 3); put_long(x, h); }               // a block's size
      x.insert(x.end(), f.begin() + (long)hdr, f.begin() + (long)hdr + 30);
      msg = scan(x.data(), x.size(), ci);
      EXPECT(!msg.empty() && msg.rfind("container: ", 0) == 0, "hostile length %lld at place %d: '%s'", (long long)h, where, msg.c_str());
    }
  }
  const uint8_t endless[12] = {0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF};
  Bytes y(f.begin(), f.begin() + 4);
  y.insert(y.end(), endless, endless + 12);
  EXPECT(!scan(y.data(), y.size(), ci).empty(), "an endless varint is accepted");
  EXPECT(scan(nullptr, 0, ci) == "container: truncated header", "the empty file");

  std::printf("container_scan_check: %zu prefixes (%zu refused), %zu bit flips (%zu refused), %zu hostile lengths, %d failures\n",
              cuts, refused, flips, flip_refused, hostile, failures);
  return failures ? 1 : 0;
}
