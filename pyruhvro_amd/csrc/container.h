// Avro object container files (rh_decode_blocks): parameters of the split kernel (container.hip), shared by
// host and device code.  Not one of the headers the specialised kernels include: the kernel-cache key does not see this file.
#pragma once
#include "program.h"
#include "filter.h"      // FilterProgram, kFilterSlots: the predicate of rh_k_split_where

namespace rh {

// Beside program.h's ErrCode, the way F_DROP lives in walk_drop.h: a block whose records do not end where the block does.
// detail = the byte of the block's payload at which its records ended.
constexpr uint32_t E_BLOCK_END = 0x100;

// What a failing lane leaves for its block (zero at launch: code 0 = the block is fine).
struct SplitErr {
  uint32_t code;     // ErrCode, or E_BLOCK_END
  uint32_t pad;
  int64_t detail;
};

// Order of the failures of one call: a malformed record r has key 2 r + 1, a block that does not end where its records do
// has key 2 first[b + 1] -- behind its own last record, in front of the next block's first.  The lowest key wins (atomicMax of
// its complement, as KParams::first_bad).
RH_HD inline unsigned long long split_key_record(uint64_t rec) { return 2ull * rec + 1ull; }
RH_HD inline unsigned long long split_key_block(uint64_t first_next) { return 2ull * first_next; }

// rh_k_split: one lane per block, 256 blocks per workgroup; the careful counters-only walk of the writer's plain program, once
// per record of the block, from global memory.
struct SParams {
  const uint8_t* data;       // the uploaded file (or the inflated blocks back to back), 16-byte aligned
  uint64_t data_len;         // readable bytes at data
  const uint64_t* start;     // [nb] first byte of every block's payload
  const uint64_t* end;       // [nb] the byte behind it (end - start < 4 GiB - 16)
  const uint64_t* first;     // [nb + 1] index of every block's first record; first[nb] = n
  uint32_t nb;
  int32_t list_depth;
  const Op* prog;
  const uint32_t* sym_off;
  const uint8_t* sym_data;
  uint64_t* offsets;         // out [n + 1]: record i spans offsets[i] .. offsets[i + 1] (a block's last record runs on to the next block's first)
  SplitErr* err;             // out [nb]
  unsigned long long* first_bad;   // [0] ~(lowest failure key), 0 if none
};

// ---- row filters in the split walk (rh_decode_blocks_where, rh_filter_blocks) ---------------------------------
// rh_k_split_where: rh_k_split whose walk also evaluates a predicate (filter_eval.h filter_walk) at the ops its terms mark.
// S.prog is the program the predicate was compiled against (the filter's own plain compile of the writer's text).
struct SWParams {
  SParams S;
  uint64_t* keep;               // [ceil(n / 64)] FParams::keep's format; ZERO at launch, filled by atomic ORs (container_where_core.h)
  unsigned long long* kept;     // [kFilterSlots] kept records, summed by the host (zero at launch)
  const uint8_t* cbytes;        // the byte comparands of the terms (FilterTerm::boff)
  const FilterProgram* flt;     // the predicate, in DEVICE memory: its terms are read where a marked op is met (filter_eval.h f_eval)
};

// ---- tolerant container reads (rh_decode_blocks_tolerant) ----------------------------------------------------
// What EVERY lane of rh_k_split_salvage leaves for its block.  A sound block: {0, 0, count, end}.  A malformed record j:
// {its ErrCode, its detail, j, the byte at which record j begins}.  Records that end before the block does: {E_BLOCK_END, the
// byte of the payload at which they ended, count, the byte behind the last record}.
struct SalvageRec {
  uint32_t code;
  uint32_t pad;
  int64_t detail;
  uint64_t kept;       // records of the block that passed
  uint64_t kept_end;   // absolute byte at which the first record that is not kept begins (start <= kept_end <= end)
};

// rh_k_split_salvage: rh_k_split whose failing lane stops its own block only.  S.err is not written; S.first_bad is (any
// non-zero value = at least one block has a code, the host then reads `rec`).
struct SalvageParams {
  SParams S;
  SalvageRec* rec;     // out [nb]
};

// One keeping block of rh_k_salvage_gather: bytes [src, src + len) of the split's buffer go to [dst, dst + len) of the gathered
// one, zeros to [dst + len, dst_next); record j < kept had offset off[off_first + j] and gets new_off[new_first + j].
struct GatherJob {
  uint64_t src, len;
  uint64_t dst, dst_next;      // dst is a multiple of 16; dst_next - (dst + len) <= 15
  uint64_t off_first, new_first, kept;
  uint64_t last;               // 1 = the last keeping block: it writes new_off[new_first + kept] = dst + len
};

// rh_k_salvage_gather: one wavefront per job.
struct SalvageGatherParams {
  const uint8_t* data;         // the split's buffer
  const uint64_t* off;         // the split's offsets
  const GatherJob* jobs;       // [njobs]
  uint32_t njobs;
  uint8_t* out;                // the gathered buffer (16-byte aligned), out_len bytes
  uint64_t out_len;
  uint64_t* new_off;           // [n' + 1]
};

}  // namespace rh
