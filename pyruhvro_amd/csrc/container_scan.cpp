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

std::string container_scan(const uint8_t* data, uint64_t len, ContainerInfo& out) {
  static const uint8_t kMagic[4] = {'O', 'b', 'j', 1};
  out = ContainerInfo();
  if (!data && len) return "container: null buffer";
  const uint64_t have = len < 4 ? len : 4;
  if (have && std::memcmp(data, kMagic, (size_t)have) != 0) return "container: bad magic (not an Avro object container file)";
  if (len < 4) return "container: truncated header";
  Reader r{data, len, 4};

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

  // the blocks: count, size, `size` bytes, the sync marker
  out.first.push_back(0);
  uint64_t n = 0;
  while (r.at < len) {
    const auto where = [&out] { return "container: block " + std::to_string(out.start.size()) + ": "; };      // (error paths only)
    int64_t cnt, size;
    if (!r.rd_long(cnt) || !r.rd_long(size)) return where() + "truncated block header (bytes left after the last complete block)";
    if (cnt < 0) return where() + "negative record count " + std::to_string(cnt);
    if (size < 0) return where() + "negative size " + std::to_string(size);
    if ((uint64_t)size > r.left()) return where() + "size " + std::to_string(size) + " runs past the end of the file";
    if ((uint64_t)cnt > (1ull << 62) - n) return where() + "record count out of range";
    const uint64_t s = r.at;
    r.at += (uint64_t)size;
    if (r.left() < 16) return where() + "truncated sync marker (bytes left after the last complete block)";
    if (std::memcmp(data + r.at, out.sync, 16) != 0) return where() + "sync marker mismatch";
    r.at += 16;
    n += (uint64_t)cnt;
    out.start.push_back(s);
    out.end.push_back(s + (uint64_t)size);
    out.first.push_back(n);
  }
  return std::string();
}

}  // namespace rhc
