// Stand-alone check of the deflate stream logic (pyruhvro_amd/csrc/inflate_core.h) for sanitizer builds: no HIP, no Python.
// Drives the core through a plain single-threaded size walk and emit walk -- every input in a heap block of exactly its own
// size, every output in a heap block of exactly the size the size walk reported, so that a read or a store outside either is a
// heap-buffer-overflow for AddressSanitizer -- and compares the verdict class, the bytes, the count of trailing bytes and the
// rule a malformed stream broke with zlib's inflate (raw, 15 window bits) over: hand-assembled streams at the edges of the
// format, zlib's own streams at several levels and strategies, every prefix of a dynamic-Huffman stream and every single-bit
// flip of it.  Exit status 0 = every verdict was zlib's.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I pyruhvro_amd/csrc
//       tools/inflate_check.cpp -o inflate_check -lz && ./inflate_check
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "inflate_core.h"

typedef std::vector<uint8_t> Bytes;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { failures++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// ---- zlib's verdict ------------------------------------------------------------------------------------------------------------
struct Verdict {
  uint32_t code = 0;
  uint64_t trailing = 0;
  std::string msg;
  Bytes out;
};

static Verdict by_zlib(const Bytes& in) {
  Verdict v;
  z_stream z;
  std::memset(&z, 0, sizeof z);
  if (inflateInit2(&z, -15) != Z_OK) std::abort();
  v.out.resize(8u << 20);
  std::unique_ptr<uint8_t[]> exact(new uint8_t[in.size() ? in.size() : 1]);
  if (!in.empty()) std::memcpy(exact.get(), in.data(), in.size());
  z.next_in = exact.get(); z.avail_in = (uInt)in.size();
  z.next_out = v.out.data(); z.avail_out = (uInt)v.out.size();
  const int rc = inflate(&z, Z_NO_FLUSH);
  if (z.avail_out == 0) { std::printf("the harness's output buffer is too small\n"); std::abort(); }
  if (rc == Z_STREAM_END) { v.trailing = z.avail_in; v.code = z.avail_in ? rhi::ST_TRAILING : rhi::ST_OK; }
  else if (rc == Z_DATA_ERROR) { v.code = rhi::ST_MALFORMED; v.msg = z.msg ? z.msg : ""; }
  else if (rc == Z_OK || rc == Z_BUF_ERROR) v.code = rhi::ST_TRUNCATED;      // (all input taken, no end of stream)
  else { std::printf("zlib: unexpected return %d\n", rc); std::abort(); }
  v.out.resize(v.out.size() - z.avail_out);
  inflateEnd(&z);
  return v;
}

// the rule(s) of inflate_core.h behind each of zlib's messages: reason, and detail (-1: any)
static bool reason_matches(const std::string& msg, const rhi::Status& s) {
  const uint32_t r = s.reason;
  const uint64_t d = s.detail;
  if (msg == "invalid block type") return r == rhi::R_BLOCK_TYPE;
  if (msg == "invalid stored block lengths") return r == rhi::R_STORED_LEN;
  if (msg == "too many length or distance symbols") return r == rhi::R_TOO_MANY;
  if (msg == "invalid code lengths set") return (r == rhi::R_OVERSUBSCRIBED || r == rhi::R_INCOMPLETE) && d == 0;
  if (msg == "invalid bit length repeat") return r == rhi::R_REPEAT;
  if (msg == "invalid code -- missing end-of-block") return r == rhi::R_NO_EOB;
  if (msg == "invalid literal/lengths set") return (r == rhi::R_OVERSUBSCRIBED || r == rhi::R_INCOMPLETE) && d == 1;
  if (msg == "invalid distances set") return (r == rhi::R_OVERSUBSCRIBED || r == rhi::R_INCOMPLETE) && d == 2;
  if (msg == "invalid literal/length code") return (r == rhi::R_NO_CODE && d == 1) || r == rhi::R_LITLEN_286;
  if (msg == "invalid distance code") return (r == rhi::R_NO_CODE && d == 2) || r == rhi::R_DIST_30;
  if (msg == "invalid distance too far back") return r == rhi::R_TOO_FAR;
  return false;
}

// ---- the core's verdict: a size walk, then an emit walk into exactly that many bytes -------------------------------------------
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

static size_t reasons_seen[rhi::R_COUNT], classes_seen[6];

static rhi::Status check(const Bytes& in, const char* what, long arg = -1, uint64_t max_out = ~0ull) {
  std::unique_ptr<uint8_t[]> exact(new uint8_t[in.size() ? in.size() : 1]);
  if (!in.empty()) std::memcpy(exact.get(), in.data(), in.size());
  const uint8_t* p = in.empty() ? nullptr : exact.get();
  std::unique_ptr<rhi::Tables> T(new rhi::Tables);
  std::memset(T.get(), 0xEE, sizeof(rhi::Tables));
  T->fixed_ready = 0;
  rhi::CountSink cs;
  const rhi::Status s = rhi::inflate_stream(p, in.size(), *T, cs, max_out, true);
  if (max_out != ~0ull) return s;
  const Verdict z = by_zlib(in);
  classes_seen[s.code < 6 ? s.code : 5]++;
  EXPECT(s.code == z.code, "%s %ld: class %u, zlib's %u (%s)", what, arg, s.code, z.code, z.msg.c_str());
  if (s.code != z.code) return s;
  if (s.code == rhi::ST_TRAILING) EXPECT(s.detail == z.trailing, "%s %ld: %llu trailing bytes, zlib's %llu", what, arg, (unsigned long long)s.detail, (unsigned long long)z.trailing);
  if (s.code == rhi::ST_MALFORMED) {
    reasons_seen[s.reason < rhi::R_COUNT ? s.reason : 0]++;
    EXPECT(reason_matches(z.msg, s), "%s %ld: reason %u detail %llu for zlib's '%s'", what, arg, s.reason, (unsigned long long)s.detail, z.msg.c_str());
  }
  if (s.code == rhi::ST_OK || s.code == rhi::ST_TRAILING) {
    EXPECT(cs.n == z.out.size(), "%s %ld: %llu bytes counted, zlib's %zu", what, arg, (unsigned long long)cs.n, z.out.size());
    std::unique_ptr<uint8_t[]> out(new uint8_t[cs.n ? cs.n : 1]);
    HostSink hs{out.get(), cs.n};
    std::memset(T.get(), 0xEE, sizeof(rhi::Tables));
    T->fixed_ready = 0;
    const rhi::Status e = rhi::inflate_stream(p, in.size(), *T, hs, max_out, true);
    EXPECT(e.code == s.code && e.detail == s.detail && hs.n == cs.n, "%s %ld: the emit walk disagrees with the size walk", what, arg);
    EXPECT(hs.n == z.out.size() && (hs.n == 0 || std::memcmp(out.get(), z.out.data(), hs.n) == 0), "%s %ld: bytes differ from zlib's", what, arg);
    if (cs.n > 1) {      // an emit walk into one byte less stops, and stores nothing outside
      std::unique_ptr<uint8_t[]> small(new uint8_t[cs.n - 1]);
      HostSink h2{small.get(), cs.n - 1};
      std::memset(T.get(), 0xEE, sizeof(rhi::Tables));
      T->fixed_ready = 0;
      const rhi::Status e2 = rhi::inflate_stream(p, in.size(), *T, h2, max_out, true);
      EXPECT(e2.code == rhi::ST_INTERNAL, "%s %ld: an emit walk past its size pass went on", what, arg);
    }
  }
  return s;
}

// ---- making streams ------------------------------------------------------------------------------------------------------------
struct BitW {
  Bytes out;
  uint32_t acc = 0, n = 0;
  void put(uint32_t v, uint32_t bits) {      // LSB first
    for (uint32_t i = 0; i < bits; i++) {
      acc |= ((v >> i) & 1u) << n;
      if (++n == 8) { out.push_back((uint8_t)acc); acc = 0; n = 0; }
    }
  }
  void huff(uint32_t code, uint32_t bits) {      // a Huffman code: most significant bit first
    for (uint32_t i = bits; i-- > 0;) put((code >> i) & 1u, 1);
  }
  void align() { if (n) put(0, 8 - n); }
  void bytes(const uint8_t* p, size_t k) { for (size_t i = 0; i < k; i++) out.push_back(p[i]); }
  Bytes done() { align(); return out; }
};

static std::vector<uint32_t> canonical(const std::vector<uint8_t>& lens) {
  uint32_t count[16] = {0}, next[16] = {0};
  for (uint8_t l : lens) count[l]++;
  count[0] = 0;
  uint32_t code = 0;
  for (int l = 1; l < 16; l++) { code = (code + count[l - 1]) << 1; next[l] = code; }
  std::vector<uint32_t> codes(lens.size(), 0);
  for (size_t i = 0; i < lens.size(); i++) if (lens[i]) codes[i] = next[lens[i]]++;
  return codes;
}

// RFC 1951 3.2.5 as it prints them
static const uint16_t kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
static const uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
static const uint16_t kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
static const uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
static const uint8_t kOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// the symbols of one block in a given pair of codes
struct Coder {
  std::vector<uint8_t> ll, dl;
  std::vector<uint32_t> lc, dc;
  BitW* w;
  void set(const std::vector<uint8_t>& l, const std::vector<uint8_t>& d) { ll = l; dl = d; lc = canonical(l); dc = canonical(d); }
  void fixed() {
    std::vector<uint8_t> l(288), d(32, 5);
    for (int i = 0; i < 288; i++) l[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
    set(l, d);
  }
  void sym(uint32_t s) { w->huff(lc[s], ll[s]); }
  void lit(const char* s) { for (; *s; s++) sym((uint8_t)*s); }
  void dist(uint32_t d) {
    int c = 29;
    while (kDistBase[c] > d) c--;
    w->huff(dc[c], dl[c]);
    w->put(d - kDistBase[c], kDistExtra[c]);
  }
  void match(uint32_t length, uint32_t d, int force_sym = -1) {
    int c = 28;
    if (force_sym >= 0) c = force_sym - 257;
    else while (kLenBase[c] > length) c--;
    sym(257 + c);
    w->put(length - kLenBase[c], kLenExtra[c]);
    dist(d);
  }
  // the dynamic header of the codes set(): every code-length symbol in a complete code of its own, the lengths of both codes
  // run-length coded as ONE sequence (a repeat may cross from the literal/length lengths into the distance lengths).
  // Returns true when a repeat did cross.
  bool header(bool final) {
    std::vector<uint8_t> cl(19);
    for (int i = 0; i < 19; i++) cl[i] = i < 13 ? 4 : 5;
    const std::vector<uint32_t> cc = canonical(cl);
    w->put(final ? 1 : 0, 1); w->put(2, 2);
    w->put((uint32_t)ll.size() - 257, 5); w->put((uint32_t)dl.size() - 1, 5); w->put(15, 4);
    for (int i = 0; i < 19; i++) w->put(cl[kOrder[i]], 3);
    std::vector<uint8_t> all(ll);
    all.insert(all.end(), dl.begin(), dl.end());
    bool crossed = false;
    for (size_t i = 0; i < all.size();) {
      size_t run = 1;
      while (i + run < all.size() && all[i + run] == all[i]) run++;
      if (all[i] == 0 && run >= 3) {
        const size_t r = run > 138 ? 138 : run;
        if (r >= 11) { w->huff(cc[18], cl[18]); w->put((uint32_t)r - 11, 7); }
        else { w->huff(cc[17], cl[17]); w->put((uint32_t)r - 3, 3); }
        if (i < ll.size() && i + r > ll.size()) crossed = true;
        i += r;
      } else if (all[i] != 0 && run >= 4) {
        w->huff(cc[all[i]], cl[all[i]]);
        const size_t r = run - 1 > 6 ? 6 : run - 1;
        w->huff(cc[16], cl[16]); w->put((uint32_t)r - 3, 2);
        if (i < ll.size() && i + r >= ll.size()) crossed = true;
        i += 1 + r;
      } else {
        w->huff(cc[all[i]], cl[all[i]]);
        i++;
      }
    }
    return crossed;
  }
};

static Bytes stored_block(const Bytes& data, bool final) {
  BitW w;
  w.put(final ? 1 : 0, 1); w.put(0, 2); w.align();
  w.put((uint32_t)data.size(), 16); w.put((uint32_t)data.size() ^ 0xFFFF, 16);
  w.bytes(data.data(), data.size());
  return w.out;
}

static uint32_t rng_state = 20260921u;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static Bytes noise(size_t n) { Bytes b(n); for (auto& x : b) x = (uint8_t)rng(); return b; }

static Bytes text(size_t n) {      // record-like: repeated field names, numbers, some noise
  std::string s;
  for (size_t i = 0; s.size() < n; i++) {
    s += "{\"name\":\"user-" + std::to_string(i * 7919 % 1000) + "\",\"age\":" + std::to_string(rng() % 90) + ",\"emails\":[\"u" + std::to_string(rng() % 50) + "@example.org\"]";
    s += i % 3 ? ",\"status\":null}" : ",\"status\":\"" + std::string(1 + rng() % 9, (char)('a' + rng() % 26)) + "\"}";
  }
  s.resize(n);
  return Bytes(s.begin(), s.end());
}

static Bytes deflate_of(const Bytes& data, int level, int strategy, const std::vector<std::pair<size_t, int>>& flushes = {}) {
  z_stream z;
  std::memset(&z, 0, sizeof z);
  if (deflateInit2(&z, level, Z_DEFLATED, -15, 8, strategy) != Z_OK) std::abort();
  Bytes out(deflateBound(&z, (uLong)data.size()) + 64 * (flushes.size() + 1) + 64);
  z.next_out = out.data(); z.avail_out = (uInt)out.size();
  size_t at = 0;
  Bytes copy(data.empty() ? Bytes(1) : data);
  for (const auto& f : flushes) {
    z.next_in = copy.data() + at; z.avail_in = (uInt)(f.first - at);
    if (deflate(&z, f.second) != Z_OK) { std::printf("deflate: flush failed\n"); std::abort(); }
    at = f.first;
  }
  z.next_in = copy.data() + at; z.avail_in = (uInt)(data.size() - at);
  if (deflate(&z, Z_FINISH) != Z_STREAM_END) { std::printf("deflate: finish failed\n"); std::abort(); }
  out.resize(out.size() - z.avail_out);
  deflateEnd(&z);
  return out;
}

int main() {
  std::setvbuf(stdout, nullptr, _IOLBF, 0);
  // the arithmetic of the base / extra-bit tables and of the permuted order against the RFC's print of them
  for (uint32_t s = 0; s < 29; s++) EXPECT(rhi::len_base(s) == kLenBase[s] && rhi::len_extra(s) == kLenExtra[s], "length symbol %u", 257 + s);
  for (uint32_t d = 0; d < 30; d++) EXPECT(rhi::dist_base(d) == kDistBase[d] && rhi::dist_extra(d) == kDistExtra[d], "distance symbol %u", d);
  for (uint32_t i = 0; i < 19; i++) EXPECT(rhi::clen_order(i) == kOrder[i], "code-length order %u", i);

  size_t hand = 0;
  auto accepted = [&](const Bytes& b, const char* what) {
    hand++;
    const rhi::Status s = check(b, what);
    EXPECT(s.code == rhi::ST_OK, "%s: not accepted (class %u reason %u)", what, s.code, s.reason);
  };
  // ---- hand-assembled, at the edges of the format
  accepted(stored_block(Bytes(), true), "stored, length 0");
  { BitW w; Coder c; c.w = &w; c.fixed(); w.put(1, 1); w.put(1, 2); c.sym(256); accepted(w.done(), "fixed, end-of-block only"); }
  accepted(stored_block(noise(65535), true), "stored, 65,535 bytes");
  {
    Bytes b = stored_block(noise(32768), false);
    BitW w; Coder c; c.w = &w; c.fixed();
    w.put(1, 1); w.put(1, 2); c.match(258, 32768); c.sym(256);
    const Bytes t = w.done();
    b.insert(b.end(), t.begin(), t.end());
    accepted(b, "32,768 stored, then length 258 at distance 32,768");
  }
  for (uint32_t d = 1; d <= 3; d++) {
    BitW w; Coder c; c.w = &w; c.fixed();
    w.put(1, 1); w.put(1, 2); c.lit("xyz"); c.match(258, d); c.lit("!"); c.match(258, d); c.sym(256);
    accepted(w.done(), "length 258 at distances 1, 2, 3");
  }
  for (int sym : {285, 284}) {
    BitW w; Coder c; c.w = &w; c.fixed();
    w.put(1, 1); w.put(1, 2); c.lit("ab"); c.match(258, 2, sym); c.sym(256);
    accepted(w.done(), "length 258 as 285 and as 284 + 31");
  }
  auto few = [](std::initializer_list<std::pair<int, int>> symlens, size_t n) {
    std::vector<uint8_t> l(n, 0);
    for (auto& p : symlens) l[(size_t)p.first] = (uint8_t)p.second;
    return l;
  };
  {      // one distance code of length 1 (an incomplete code zlib lets through), used
    BitW w; Coder c; c.w = &w;
    c.set(few({{'a', 2}, {'b', 2}, {256, 2}, {260, 2}}, 261), few({{3, 1}}, 4));
    c.header(true); c.lit("abab"); c.match(6, 4); c.sym(256);
    accepted(w.done(), "dynamic, one distance code of length 1");
  }
  {      // no distance code at all, none used
    BitW w; Coder c; c.w = &w;
    c.set(few({{'a', 1}, {'b', 2}, {256, 2}}, 257), few({}, 1));
    c.header(true); c.lit("abba"); c.sym(256);
    accepted(w.done(), "dynamic, no distance code");
  }
  {      // ... and a match in such a block is refused as zlib refuses it
    BitW w; Coder c; c.w = &w;
    c.set(few({{'a', 2}, {'b', 2}, {256, 2}, {257, 2}}, 258), few({}, 1));
    c.header(true); c.lit("abba"); c.sym(257); w.put(0, 8);
    hand++;
    EXPECT(check(w.done(), "dynamic, no distance code, a match").reason == rhi::R_NO_CODE, "a distance with no distance code");
  }
  {      // codes of 1 .. 15 bits
    std::vector<uint8_t> l(257, 0);
    for (int i = 0; i < 14; i++) l[(size_t)('a' + i)] = (uint8_t)(i + 1);
    l['o'] = 15; l[256] = 15;
    BitW w; Coder c; c.w = &w;
    c.set(l, few({{0, 1}, {1, 1}}, 2));
    c.header(true); c.lit("abcdefghijklmnoonmlkjihgfedcba"); c.sym(256);
    accepted(w.done(), "dynamic, a 15-bit code");
  }
  {      // a length repeat that runs from the literal/length lengths into the distance lengths
    BitW w; Coder c; c.w = &w;
    c.set(few({{'a', 2}, {'b', 2}, {256, 2}, {257, 2}}, 258), few({{0, 2}, {1, 2}, {2, 2}, {3, 2}}, 4));
    const bool crossed = c.header(true);
    EXPECT(crossed, "the repeat did not cross the HLIT boundary");
    c.lit("abab"); c.match(3, 4); c.match(3, 1); c.sym(256);
    accepted(w.done(), "dynamic, a repeat across the HLIT boundary");
  }
  {      // many deflate blocks, sync and full flushes between them, ending off a byte boundary; history across blocks
    const Bytes t = text(9000);
    const Bytes s = deflate_of(t, 6, Z_DEFAULT_STRATEGY, {{1000, Z_SYNC_FLUSH}, {1001, Z_FULL_FLUSH}, {4000, Z_SYNC_FLUSH}, {4003, Z_SYNC_FLUSH}, {7777, Z_FULL_FLUSH}});
    accepted(s, "many deflate blocks");
  }
  // ---- hand-assembled, one per rule that a flipped stream seldom breaks
  auto refused = [&](const Bytes& b, uint32_t rule, const char* what) {
    hand++;
    const rhi::Status s = check(b, what);
    EXPECT(s.code == rhi::ST_MALFORMED && s.reason == rule, "%s: class %u reason %u", what, s.code, s.reason);
  };
  refused(Bytes{0x07}, rhi::R_BLOCK_TYPE, "block type 3");
  refused(Bytes{0x01, 0x05, 0x00, 0x05, 0x00, 1, 2, 3, 4, 5}, rhi::R_STORED_LEN, "stored, LEN != ~NLEN");
  { BitW w; w.put(1, 1); w.put(2, 2); w.put(30, 5); w.put(0, 5); w.put(0, 4); w.put(0, 32); refused(w.done(), rhi::R_TOO_MANY, "287 literal/length symbols"); }
  { BitW w; w.put(1, 1); w.put(2, 2); w.put(0, 5); w.put(30, 5); w.put(0, 4); w.put(0, 32); refused(w.done(), rhi::R_TOO_MANY, "31 distance symbols"); }
  for (uint32_t s : {286u, 287u}) { BitW w; Coder c; c.w = &w; c.fixed(); w.put(1, 1); w.put(1, 2); c.lit("a"); c.sym(s); w.put(0, 16); refused(w.done(), rhi::R_LITLEN_286, "literal/length symbol 286 / 287"); }
  for (uint32_t d : {30u, 31u}) { BitW w; Coder c; c.w = &w; c.fixed(); w.put(1, 1); w.put(1, 2); c.lit("abc"); c.sym(257); w.huff(d, 5); w.put(0, 16); refused(w.done(), rhi::R_DIST_30, "distance symbol 30 / 31"); }
  { BitW w; Coder c; c.w = &w; c.fixed(); w.put(1, 1); w.put(1, 2); c.lit("ab"); c.match(3, 3); c.sym(256); refused(w.done(), rhi::R_TOO_FAR, "distance 3 behind 2 bytes"); }
  {      // ... across blocks the history counts: the same match behind a stored block of one byte is accepted
    Bytes b = stored_block(Bytes{'z'}, false);
    BitW w; Coder c; c.w = &w; c.fixed(); w.put(1, 1); w.put(1, 2); c.lit("ab"); c.match(3, 3); c.sym(256);
    const Bytes t = w.done();
    b.insert(b.end(), t.begin(), t.end());
    accepted(b, "history across deflate blocks");
  }
  // ---- zlib's own
  size_t made = 0;
  const Bytes twice = [] { Bytes a = noise(40000), b = a; b.insert(b.end(), a.begin(), a.end()); return b; }();
  const Bytes inputs[] = {text(30000), Bytes(100000, 0), noise(70000), twice, Bytes(), Bytes(1, 'x')};
  for (const Bytes& in : inputs)
    for (int level : {0, 1, 6, 9})
      for (int strategy : {Z_DEFAULT_STRATEGY, Z_FIXED, Z_RLE, Z_HUFFMAN_ONLY}) {
        made++;
        const rhi::Status s = check(deflate_of(in, level, strategy), "zlib-made stream", (long)made);
        EXPECT(s.code == rhi::ST_OK, "zlib-made stream %zu: class %u", made, s.code);
      }
  // ---- damage: every prefix and every single-bit flip of a dynamic-Huffman stream; prefixes of refused flips
  const Bytes dyn = deflate_of(text(1200), 9, Z_DEFAULT_STRATEGY);
  EXPECT((dyn[0] & 7) == 5, "the damage stream does not start with a final dynamic block");
  size_t prefixes = 0, flips = 0, flip_prefixes = 0;
  for (size_t cut = 0; cut < dyn.size(); cut++, prefixes++)
    EXPECT(check(Bytes(dyn.begin(), dyn.begin() + (long)cut), "prefix", (long)cut).code == rhi::ST_TRUNCATED, "prefix of %zu bytes is not truncated", cut);
  Bytes g = dyn;
  size_t taken = 0;
  for (size_t i = 0; i < dyn.size(); i++)
    for (int bit = 0; bit < 8; bit++, flips++) {
      g[i] ^= (uint8_t)(1u << bit);
      const rhi::Status s = check(g, "flip", (long)(i * 8 + (size_t)bit));
      if (s.code == rhi::ST_MALFORMED && flips % 37 == 0 && taken < 24) {
        taken++;
        for (size_t cut = 0; cut < g.size(); cut++, flip_prefixes++) check(Bytes(g.begin(), g.begin() + (long)cut), "prefix of a refused flip", (long)cut);
      }
      g[i] ^= (uint8_t)(1u << bit);
    }
  // two bytes behind a whole stream, and the limit: refused at it, accepted one above it
  {
    Bytes t = dyn;
    t.push_back(0); t.push_back(1);
    const rhi::Status s = check(t, "trailing");
    EXPECT(s.code == rhi::ST_TRAILING && s.detail == 2, "two bytes behind the stream");
    for (const Bytes& b : {dyn, stored_block(noise(1200), true)}) {
      EXPECT(check(b, "limit", 1200, 1200).code == rhi::ST_TOO_LARGE, "a block of exactly the limit is accepted");
      EXPECT(check(b, "limit", 1201, 1201).code == rhi::ST_OK, "a block of one byte less than the limit is refused");
    }
  }
  for (int c = rhi::ST_OK; c <= rhi::ST_TRAILING; c++) EXPECT(classes_seen[c] > 0, "class %d never met", c);
  for (uint32_t r = 1; r < rhi::R_COUNT; r++) EXPECT(reasons_seen[r] > 0, "rule %u never met", r);

  std::printf("inflate_check: %zu hand-assembled, %zu zlib-made, %zu prefixes, %zu bit flips, %zu prefixes of refused flips; classes ok/malformed/truncated/trailing %zu/%zu/%zu/%zu; rules",
              hand, made, prefixes, flips, flip_prefixes, classes_seen[0], classes_seen[1], classes_seen[2], classes_seen[3]);
  for (uint32_t r = 1; r < rhi::R_COUNT; r++) std::printf(" %u:%zu", r, reasons_seen[r]);
  std::printf("; %d failures\n", failures);
  return failures ? 1 : 0;
}
