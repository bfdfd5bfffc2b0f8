// Framing of an Avro object container file (Avro 1.11 "Object Container Files"): the header and the block
// table, from untrusted bytes.  Plain C++ with no HIP include -- it also compiles into a stand-alone program
// (tools/container_scan_check.cpp).
#pragma once
#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

namespace rhc {

struct ContainerInfo {
  std::string schema;                    // metadata entry "avro.schema", verbatim
  std::string codec;                     // "avro.codec"; absent = "null"
  uint8_t sync[16] = {0};
  std::vector<std::pair<std::string, std::string>> metadata;   // the other entries, in file order (values are bytes)
  // the block table: payload of block b = bytes [start[b], end[b]) of the file, its first record has index first[b]
  std::vector<uint64_t> start, end;      // [nb]
  std::vector<uint64_t> first;           // [nb + 1]; first[nb] = n
  uint64_t nb() const { return start.size(); }
  uint64_t n() const { return first.empty() ? 0 : first.back(); }
};

// Parses data[0 .. len).  Every read is checked against `len`.  Returns "" and fills `out`, or a message that starts with
// "container: " (and names the block index where there is one); `out` is then unspecified.
std::string container_scan(const uint8_t* data, uint64_t len, ContainerInfo& out);

// What the salvage scan finds in a damaged file: the blocks that are framed -- count >= 0, size >= 0 that fits
// in the file, the file's sync marker behind the payload -- and the gaps between them.  Blocks and gaps are ascending, disjoint,
// and tile [header_end, len) exactly.
struct SalvageInfo {
  ContainerInfo info;                    // the header; the table of the framed blocks
  uint64_t header_end = 0;               // the byte behind the header's sync marker
  std::vector<uint64_t> header_offset;   // [nb] the first byte of the block's header (its payload ends 16 bytes before the next thing)
  std::vector<uint64_t> count;           // [nb] the count the block's header claims
  std::vector<uint8_t> refused;          // [nb] 1 = "record count out of range": the count is not in info.first (it counts as 0 there)
  struct Gap {
    uint64_t offset, length;             // the bytes skipped: from the block header that could not be framed to behind the next marker (or to len)
    uint64_t block;                      // blocks framed in front of it
    std::string message;                 // what container_scan says at `offset`
  };
  std::vector<Gap> gaps;
  uint64_t steps = 0;                    // loop turns of the scan (outer and search), for the linearity check
};

// container_scan that goes on past a block it cannot frame: it searches for the next occurrence of the sync marker at or after
// the failing block header and frames again behind it.  Fails (a message, as container_scan) for a header that does not parse
// only.  Where container_scan succeeds, out.info is what it fills and there are no gaps.  Every read is checked against `len`;
// the work is O(len) whatever the bytes are.
std::string container_salvage(const uint8_t* data, uint64_t len, SalvageInfo& out);

}  // namespace rhc
