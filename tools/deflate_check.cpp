// Stand-alone check of the deflate WRITER's stream logic (pyruhvro_amd/csrc/deflate_core.h) for sanitizer builds: no HIP, no
// Python.  Every input sits in a heap block of exactly its size and every output in one of exactly deflate_bound bytes, so that
// a read or a store outside either is a heap-buffer-overflow for AddressSanitizer.  For every input x every strategy: zlib's
// inflate (raw, 15 window bits) returns the input with avail_in == 0 at Z_STREAM_END, the size is within the bound, and the
// project's own inflate_core walk accepts the stream and returns the same bytes.  The code builder is driven directly too:
// Fibonacci histograms that need more than 15 (and, for the code-length code, more than 7) bits unlimited, histograms with 0, 1
// and 2 used distance symbols, the length limit and Kraft equality of every code that must be complete.  Exit status 0 = clean.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I pyruhvro_amd/csrc
//       tools/deflate_check.cpp -o deflate_check -lz && ./deflate_check
//
//   deflate_check --ratio FILE...    each file as one stream: the same checks under every strategy, and the sizes of this
//                                    writer (AUTO), zlib level 1 and zlib level 1 Z_FIXED
#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "deflate_core.h"

typedef std::vector<uint8_t> Bytes;

static int failures = 0;
static size_t streams = 0, forms_seen[3], fallbacks = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { failures++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// ---- generators ----------------------------------------------------------------------------------------------------------------
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}
static Bytes noise(size_t n) {
  Bytes b(n);
  for (auto& v : b) v = (uint8_t)rnd();
  return b;
}
static Bytes text(size_t n) {
  Bytes out;
  char line[256];
  for (unsigned i = 0; out.size() < n; i++) {
    const int k = std::snprintf(line, sizeof line, "{\"name\":\"user-%u\",\"age\":%u,\"emails\":[\"u%u@example.org\"],\"status\":%s}", i * 7919 % 1000, rnd() % 90,
                                rnd() % 50, i % 3 ? "null" : "\"ok\"");
    out.insert(out.end(), line, line + k);
  }
  out.resize(n);
  return out;
}
static Bytes repeat(const Bytes& unit, size_t times) {
  Bytes out;
  for (size_t i = 0; i < times; i++) out.insert(out.end(), unit.begin(), unit.end());
  return out;
}
static Bytes cat(Bytes a, const Bytes& b, size_t nb) {
  a.insert(a.end(), b.begin(), b.begin() + nb);
  return a;
}
static Bytes fibonacci_bytes() {      // byte frequencies 1, 1, 2, 3, 5, ... over 20 values, shuffled
  Bytes out;
  uint32_t a = 1, b = 1;
  for (int v = 0; v < 20; v++) {
    out.insert(out.end(), a, (uint8_t)(v * 11 + 3));
    const uint32_t c = a + b; a = b; b = c;
  }
  for (size_t i = out.size() - 1; i > 0; i--) std::swap(out[i], out[rnd() % (i + 1)]);
  return out;
}

// ---- one stream ----------------------------------------------------------------------------------------------------------------
struct HostSink {
  uint8_t* buf;
  uint64_t size, n = 0;
  bool lit(uint8_t v) { if (n >= size) return false; buf[n++] = v; return true; }
  bool copy(uint32_t length, uint32_t dist) {
    if (length > size - n) return false;
    for (uint32_t i = 0; i < length; i++, n++) buf[n] = buf[n - dist];
    return true;
  }
  bool stored(const uint8_t* src, uint32_t k) {
    if (k > size - n) return false;
    if (k) std::memcpy(buf + n, src, k);
    n += k;
    return true;
  }
  uint64_t produced() const { return n; }
};

static std::unique_ptr<rhd::State> g_state(new rhd::State);

// -> the stream's size
static uint64_t check(const Bytes& in, uint32_t strategy, const char* what, long arg = -1) {
  streams++;
  const uint64_t bound = rhd::deflate_bound(in.size());
  EXPECT(bound <= in.size() + 16 * (in.size() / 32768 + 1), "%s %ld: the bound %llu breaks the inequality", what, arg, (unsigned long long)bound);
  std::unique_ptr<uint8_t[]> exact(new uint8_t[in.size() ? in.size() : 1]);
  if (!in.empty()) std::memcpy(exact.get(), in.data(), in.size());
  std::unique_ptr<uint8_t[]> out(new uint8_t[bound]);
  std::memset(g_state.get(), 0xEE, sizeof(rhd::State));      // nothing in State is kept between streams
  const uint64_t size = rhd::deflate_stream_host(*g_state, exact.get(), in.size(), strategy, out.get());
  EXPECT(size != ~0ull && size <= bound, "%s %ld strategy %u: size %llu, bound %llu", what, arg, strategy, (unsigned long long)size, (unsigned long long)bound);
  if (size > bound) return size;
  // which form the first block took
  const uint32_t type = (out[0] >> 1) & 3;
  EXPECT(type < 3, "%s %ld: block type 3", what, arg);
  if (type < 3) forms_seen[type]++;
  if (strategy >= rhd::FIXED && type == 0) fallbacks++;
  if (strategy == rhd::STORED) EXPECT(type == 0, "%s %ld: STORED wrote type %u", what, arg, type);
  // zlib
  std::unique_ptr<uint8_t[]> comp(new uint8_t[size ? size : 1]);
  std::memcpy(comp.get(), out.get(), size);
  Bytes back(in.size() + 1);
  z_stream z;
  std::memset(&z, 0, sizeof z);
  if (inflateInit2(&z, -15) != Z_OK) std::abort();
  z.next_in = comp.get(); z.avail_in = (uInt)size;
  z.next_out = back.data(); z.avail_out = (uInt)back.size();
  const int rc = inflate(&z, Z_FINISH);
  EXPECT(rc == Z_STREAM_END, "%s %ld strategy %u: zlib returns %d (%s)", what, arg, strategy, rc, z.msg ? z.msg : "");
  EXPECT(z.avail_in == 0, "%s %ld strategy %u: %u bytes behind the end of the stream", what, arg, strategy, z.avail_in);
  EXPECT(z.total_out == in.size() && (in.empty() || !std::memcmp(back.data(), in.data(), in.size())), "%s %ld strategy %u: zlib returns other bytes", what, arg,
         strategy);
  inflateEnd(&z);
  // the project's own inflater
  std::unique_ptr<rhi::Tables> T(new rhi::Tables);
  std::memset(T.get(), 0xEE, sizeof(rhi::Tables));
  T->fixed_ready = 0;
  std::unique_ptr<uint8_t[]> own(new uint8_t[in.size() ? in.size() : 1]);
  HostSink hs{own.get(), in.size()};
  const rhi::Status s = rhi::inflate_stream(comp.get(), size, *T, hs, ~0ull, true);
  EXPECT(s.code == rhi::ST_OK, "%s %ld strategy %u: inflate_core says class %u reason %u", what, arg, strategy, s.code, s.reason);
  EXPECT(hs.n == in.size() && (in.empty() || !std::memcmp(own.get(), in.data(), in.size())), "%s %ld strategy %u: inflate_core returns other bytes", what, arg,
         strategy);
  return size;
}

static void check_all(const Bytes& in, const char* what, long arg = -1) {
  for (uint32_t s = 0; s < 4; s++) check(in, s, what, arg);
}

// ---- the code builder ----------------------------------------------------------------------------------------------------------
static uint64_t kraft(const uint8_t* lens, uint32_t n, uint32_t maxbits, uint32_t* used, uint32_t* longest) {
  uint64_t sum = 0;
  *used = 0; *longest = 0;
  for (uint32_t i = 0; i < n; i++)
    if (lens[i]) { sum += 1ull << (maxbits - lens[i]); (*used)++; if (lens[i] > *longest) *longest = lens[i]; }
  return sum;
}

static void check_builder() {
  uint32_t key[288];
  uint16_t sym[288], freq[288];
  uint8_t lens[288];
  uint32_t used, longest;
  for (uint32_t n = 17; n <= 40; n++) {      // Fibonacci frequencies: the unlimited code needs n - 1 bits
    std::memset(freq, 0, sizeof freq);
    uint32_t a = 1, b = 1;
    for (uint32_t i = 0; i < n; i++) { freq[(i * 7) % 286] = (uint16_t)(a > 60000 ? 60000 : a); const uint32_t c = a + b; a = b; b = c; }
    const uint32_t m = rhd::build_lengths(freq, 286, 15, true, lens, key, sym);
    const uint64_t k = kraft(lens, 286, 15, &used, &longest);
    EXPECT(m == n && used == n && longest <= 15 && k == 1ull << 15, "fibonacci %u: %u codes, longest %u, kraft %llu", n, used, longest, (unsigned long long)k);
    if (n <= 24) EXPECT(longest == 15, "fibonacci %u: the limit was not needed (longest %u)", n, longest);
    for (uint32_t i = 0; i < 286; i++) EXPECT((lens[i] != 0) == (freq[i] != 0), "fibonacci %u: symbol %u", n, i);
  }
  for (uint32_t n = 9; n <= 19; n++) {      // the code-length code: 7 bits
    std::memset(freq, 0, sizeof freq);
    uint32_t a = 1, b = 1;
    for (uint32_t i = 0; i < n; i++) { freq[i] = (uint16_t)a; const uint32_t c = a + b; a = b; b = c; }
    rhd::build_lengths(freq, 19, 7, true, lens, key, sym);
    const uint64_t k = kraft(lens, 19, 7, &used, &longest);
    EXPECT(used == n && longest <= 7 && k == 1ull << 7, "clen fibonacci %u: %u codes, longest %u, kraft %llu", n, used, longest, (unsigned long long)k);
  }
  // distance histograms with 0, 1 and 2 used symbols; a literal/length histogram with one (padded to two)
  std::memset(freq, 0, sizeof freq);
  EXPECT(rhd::build_lengths(freq, 30, 15, false, lens, key, sym) == 0 && kraft(lens, 30, 15, &used, &longest) == 0, "no distance symbol");
  freq[7] = 5;
  EXPECT(rhd::build_lengths(freq, 30, 15, false, lens, key, sym) == 1 && lens[7] == 1 && kraft(lens, 30, 15, &used, &longest) == 1ull << 14 && used == 1,
         "one distance symbol");
  freq[29] = 1;
  EXPECT(rhd::build_lengths(freq, 30, 15, false, lens, key, sym) == 2 && lens[7] == 1 && lens[29] == 1, "two distance symbols");
  std::memset(freq, 0, sizeof freq);
  freq[256] = 1;
  EXPECT(rhd::build_lengths(freq, 286, 15, true, lens, key, sym) == 2 && lens[256] == 1 && lens[0] == 1 && kraft(lens, 286, 15, &used, &longest) == 1ull << 15,
         "one literal/length symbol is padded to a complete code");
  freq[0] = 3;
  EXPECT(rhd::build_lengths(freq, 286, 15, true, lens, key, sym) == 2 && lens[256] == 1 && lens[0] == 1 && lens[1] == 0, "two literal/length symbols");
  // random histograms
  for (int t = 0; t < 2000; t++) {
    std::memset(freq, 0, sizeof freq);
    const uint32_t n = 2 + rnd() % 285, shape = rnd() % 3;
    for (uint32_t i = 0; i < n; i++) freq[rnd() % 286] = (uint16_t)(shape == 0 ? 1 + rnd() % 4 : shape == 1 ? 1 + rnd() % 4000 : 1u << (rnd() % 13));
    rhd::build_lengths(freq, 286, 15, true, lens, key, sym);
    const uint64_t k = kraft(lens, 286, 15, &used, &longest);
    EXPECT(longest <= 15 && k == 1ull << 15, "random histogram %d: longest %u, kraft %llu", t, longest, (unsigned long long)k);
  }
  // the symbol of every length and distance, against the tables of RFC 1951 3.2.5 (inflate_core.h holds them as arithmetic)
  for (uint32_t l = 3; l <= 258; l++) {
    const uint32_t s = rhd::len_sym(l);
    EXPECT(s <= 28 && rhi::len_base(s) <= l && l - rhi::len_base(s) < (1u << rhi::len_extra(s)), "length %u: symbol %u", l, s);
  }
  for (uint32_t d = 1; d <= 32768; d++) {
    const uint32_t s = rhd::dist_sym(d);
    EXPECT(s <= 29 && rhi::dist_base(s) <= d && d - rhi::dist_base(s) < (1u << rhi::dist_extra(s)), "distance %u: symbol %u", d, s);
  }
}

static Bytes read_file(const char* path) {
  Bytes b;
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::printf("cannot open %s\n", path); std::exit(2); }
  uint8_t buf[65536];
  size_t k;
  while ((k = std::fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + k);
  std::fclose(f);
  return b;
}

static size_t by_zlib(const Bytes& in, int strategy) {
  z_stream z;
  std::memset(&z, 0, sizeof z);
  if (deflateInit2(&z, 1, Z_DEFLATED, -15, 8, strategy) != Z_OK) std::abort();
  Bytes out(deflateBound(&z, (uLong)in.size()) + 64);
  z.next_in = const_cast<uint8_t*>(in.data()); z.avail_in = (uInt)in.size();
  z.next_out = out.data(); z.avail_out = (uInt)out.size();
  if (deflate(&z, Z_FINISH) != Z_STREAM_END) std::abort();
  const size_t n = z.total_out;
  deflateEnd(&z);
  return n;
}

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "--ratio")) {
    for (int i = 2; i < argc; i++) {
      const Bytes in = read_file(argv[i]);
      const uint64_t ours = check(in, rhd::AUTO, argv[i]);
      for (uint32_t s = rhd::STORED; s <= rhd::DYNAMIC; s++) check(in, s, argv[i]);
      const size_t z1 = by_zlib(in, Z_DEFAULT_STRATEGY), zf = by_zlib(in, Z_FIXED);
      std::printf("%s: %zu bytes -> this writer %llu, zlib level 1 %zu, zlib level 1 Z_FIXED %zu, ratio to zlib level 1 %.4f\n", argv[i], in.size(),
                  (unsigned long long)ours, z1, zf, (double)ours / (double)z1);
    }
    return failures ? 1 : 0;
  }
  const uint32_t K = rhd::kSegment;
  check_builder();
  for (size_t n = 0; n <= 4; n++) check_all(text(n), "short", (long)n);
  for (size_t n : {257u, 258u, 259u, 260u, 517u}) check_all(Bytes(n, 0x41), "one byte repeated", (long)n);
  check_all(repeat({'a', 'b'}, 130), "ab * 130");
  {
    Bytes all(256);
    for (int i = 0; i < 256; i++) all[i] = (uint8_t)i;
    check_all(repeat(all, 2), "every byte, twice");
  }
  { const Bytes n = noise(32768); check_all(cat(n, n, 300), "distance 32768"); }
  { const Bytes n = noise(32769); check_all(cat(n, n, 300), "distance 32769"); }
  for (size_t n : {65535u, 65536u, 65537u}) check_all(noise(n), "noise", (long)n);
  for (size_t n : {K - 1, K, K + 1, 2 * K + 3}) check_all(text(n), "text", (long)n);
  check_all(Bytes(3 * K + 5, 0), "zeros");
  check_all(fibonacci_bytes(), "fibonacci bytes");
  check_all(text(200000), "text", 200000);
  {      // matches everywhere: a short phrase repeated with a counter
    Bytes b;
    for (unsigned i = 0; b.size() < 2 * K + 100; i++) { const Bytes t = text(40 + i % 7); b.insert(b.end(), t.begin(), t.end()); b.push_back((uint8_t)i); }
    check_all(b, "repeated phrase");
  }
  const uint32_t alphabets[5] = {1, 2, 4, 16, 256};
  for (int t = 0; t < 3000; t++) {
    const uint32_t a = alphabets[t % 5];
    size_t n = rnd() % 4 == 0 ? rnd() % (3 * K + 1) : rnd() % 3000;
    if (t % 97 == 0) n = 3 * K;
    Bytes b(n);
    const uint32_t runs = rnd() % 3;      // 0: independent bytes; otherwise runs and copies, so that matches of every kind occur
    for (size_t i = 0; i < n;) {
      if (runs && i > 8 && rnd() % 4 == 0) {
        const size_t back = 1 + rnd() % (i < 40000 ? i : 40000), len = 3 + rnd() % (runs == 1 ? 20 : 400);
        for (size_t k = 0; k < len && i < n; k++, i++) b[i] = b[i - back];
      } else {
        b[i++] = (uint8_t)((rnd() % a) * (a == 256 ? 1 : 37));
      }
    }
    check_all(b, "random", t);
  }
  EXPECT(forms_seen[0] && forms_seen[1] && forms_seen[2], "forms seen: stored %zu fixed %zu dynamic %zu", forms_seen[0], forms_seen[1], forms_seen[2]);
  std::printf("deflate_check: %zu streams, first blocks stored %zu / fixed %zu / dynamic %zu, %zu forced strategies fell back to stored, %d failures\n", streams,
              forms_seen[0], forms_seen[1], forms_seen[2], fallbacks, failures);
  return failures ? 1 : 0;
}
