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

}  // namespace rhc
