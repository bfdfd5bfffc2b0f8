// Avro object container framing (container_scan.h).  Untrusted input: no read without a bounds check.
#include "container_scan.h"

#include <cstring>

namespace rhc {

namespace {

struct Reader {
  const uint8_t* p;
  uint64_t len, at;
  uint64_t left() const { return len - at; }
  // zigzag long; false = the bytes ran out, or an 11th byte
  bool rd_long(int64_t& out) {
    uint64_t r = 0;
    for (uint32_t shift = 0; shift < 70; shift += 7) {
      if (at >= len) return false;
      const uint8_t b = p[at++];
      r |= (uint64_t)(b & 0x7F) << (shift < 64 ? shift : 63);
      if (!(b & 0x80)) {
        out = (int64_t)(r >> 1) ^ -(int64_t)(r & 1);
        return true;
      }
    }
    return false;
  }
  // length-prefixed bytes
  bool rd_bytes(std::string& out) {
    int64_t n;
    if (!rd_long(n) || n < 0 || (uint64_t)n > left()) return false;
    out.assign(reinterpret_cast<const char*>(p + at), (size_t)n);
    at += (uint64_t)n;
    return true;
  }
};

std::string quoted(const std::string& s) {
  std::string o = "'";
  for (size_t i = 0; i < s.size() && i < 64; i++) {
    const unsigned char ch = (unsigned char)s[i];
    o += (ch >= 0x20 && ch < 0x7F && ch != '\'') ? (char)ch : '?';
  }
  return o + "'";
}

}  // namespace

// The header: magic, the metadata map, the sync marker.  "" and r.at behind the marker, or the message.
static std::string scan_header(const uint8_t* data, uint64_t len, ContainerInfo& out, Reader& r) {
  static const uint8_t kMagic[4] = {'O', 'b', 'j', 1};
  out = ContainerInfo();
  if (!data && len) return "container: null buffer";
  const uint64_t have = len < 4 ? len : 4;
  if (have && std::memcmp(data, kMagic, (size_t)have) != 0) return "container: bad magic (not an Avro object container file)";
  if (len < 4) return "container: truncated header";
  r = Reader{data, len, 4};

  // the metadata map: blocks of (key, value) pairs, a negative count carries the block's byte size, 0 ends the map
  bool has_schema = false, has_codec = false;
  for (;;) {
    int64_t cnt;
    if (!r.rd_long(cnt)) return "container: truncated header";
    if (cnt == 0) break;
    if (cnt < 0) {
      int64_t bytes;
      if (!r.rd_long(bytes)) return "container: truncated header";
      if (bytes < 0 || cnt == INT64_MIN) return "container: malformed header (metadata block size)";
      cnt = -cnt;
    }
    if ((uint64_t)cnt > r.left() / 2) return "container: truncated header";      // (an entry is two bytes at least)
    for (int64_t i = 0; i < cnt; i++) {
      std::string key, value;
      if (!r.rd_bytes(key) || !r.rd_bytes(value)) return "container: truncated header";
      if (key == "avro.schema") { out.schema = std::move(value); has_schema = true; }
      else if (key == "avro.codec") { out.codec = std::move(value); has_codec = true; }
      else out.metadata.emplace_back(std::move(key), std::move(value));
    }
  }
  if (r.left() < 16) return "container: truncated header";
  std::memcpy(out.sync, data + r.at, 16);
  r.at += 16;
  if (!has_schema) return "container: no avro.schema in the header";
  if (!has_codec) out.codec = "null";
  if (out.codec != "null" && out.codec != "deflate") return "container: codec " + quoted(out.codec) + " is not supported";
  return std::string();
}

// One block at r.at: count, size, `size` bytes, the sync marker.  "" = framed: payload [s, e), r.at behind the marker; else the
// message, r.at unspecified.  `b`: the block's index, `n`: the records in front of it.  A count that `n` cannot take is left in
// `range` when the block is framed all the same (the strict scan refuses it, the salvage scan reports the block).
static std::string frame_block(Reader& r, const uint8_t* sync, uint64_t b, uint64_t n, int64_t& cnt, uint64_t& s, uint64_t& e, std::string& range) {
  const auto where = [b] { return "container: block " + std::to_string(b) + ": "; };      // (error paths only)
  int64_t size;
  range.clear();
  if (!r.rd_long(cnt) || !r.rd_long(size)) return where() + "truncated block header (bytes left after the last complete block)";
  if (cnt < 0) return where() + "negative record count " + std::to_string(cnt);
  if (size < 0) return where() + "negative size " + std::to_string(size);
  if ((uint64_t)size > r.left()) return where() + "size " + std::to_string(size) + " runs past the end of the file";
  if ((uint64_t)cnt > (1ull << 62) - n) range = where() + "record count out of range";
  s = r.at;
  r.at += (uint64_t)size;
  e = r.at;
  if (r.left() < 16) return !range.empty() ? range : where() + "truncated sync marker (bytes left after the last complete block)";
  if (std::memcmp(r.p + r.at, sync, 16) != 0) return !range.empty() ? range : where() + "sync marker mismatch";
  r.at += 16;
  return std::string();
}

std::string container_scan(const uint8_t* data, uint64_t len, ContainerInfo& out) {
  Reader r{data, len, 0};
  const std::string bad_header = scan_header(data, len, out, r);
  if (!bad_header.empty()) return bad_header;

  out.first.push_back(0);
  uint64_t n = 0;
  while (r.at < len) {
    int64_t cnt;
    uint64_t s, e;
    std::string range;
    const std::string bad = frame_block(r, out.sync, out.start.size(), n, cnt, s, e, range);
    if (!bad.empty()) return bad;
    if (!range.empty()) return range;
    n += (uint64_t)cnt;
    out.start.push_back(s);
    out.end.push_back(e);
    out.first.push_back(n);
  }
  return std::string();
}

// Termination and cost.  `at` is the only cursor and every turn of the outer loop moves it forward: a framed block by its
// header, payload and marker (18 bytes at least); a gap by at least 16 bytes (the marker found at q >= P puts `at` at q + 16),
// or to `len`, which ends the loop.  One turn costs one framing attempt -- at most two varints of 10 bytes and one 16-byte
// compare, wherever the claimed size points, since the payload itself is never read -- plus, in a gap, the search.  A search
// starts at the gap's P and ends at the marker it finds (or at len); the next one starts at or behind q + 16, so no byte is
// the start of a compare in two searches.  Turns <= len / 16 + 1, compares <= len, each of 16 bytes at most: O(len).
std::string container_salvage(const uint8_t* data, uint64_t len, SalvageInfo& out) {
  out = SalvageInfo();
  ContainerInfo& ci = out.info;
  Reader r{data, len, 0};
  const std::string bad_header = scan_header(data, len, ci, r);
  if (!bad_header.empty()) return bad_header;
  out.header_end = r.at;

  ci.first.push_back(0);
  uint64_t n = 0;
  while (r.at < len) {
    out.steps++;
    const uint64_t P = r.at;
    int64_t cnt;
    uint64_t s, e;
    std::string range;
    std::string bad = frame_block(r, ci.sync, ci.start.size(), n, cnt, s, e, range);
    if (bad.empty()) {
      const bool refused = !range.empty();
      if (!refused) n += (uint64_t)cnt;
      ci.start.push_back(s);
      ci.end.push_back(e);
      ci.first.push_back(n);
      out.header_offset.push_back(P);
      out.count.push_back((uint64_t)cnt);
      out.refused.push_back(refused ? 1 : 0);
      continue;
    }
    // a gap from P: to behind the next marker at or after P, or to the end of the file
    uint64_t q = P;
    bool found = false;
    while (len - q >= 16) {      // (q <= len throughout)
      out.steps++;
      const void* hit = std::memchr(data + q, ci.sync[0], (size_t)(len - q - 15));      // first bytes that have 16 bytes from them
      if (!hit) break;
      q = (uint64_t)((const uint8_t*)hit - data);
      if (std::memcmp(data + q, ci.sync, 16) == 0) { found = true; break; }
      q++;
    }
    const uint64_t resume = found ? q + 16 : len;
    out.gaps.push_back(SalvageInfo::Gap{P, resume - P, ci.start.size(), std::move(bad)});
    r.at = resume;
  }
  return std::string();
}

}  // namespace rhc
