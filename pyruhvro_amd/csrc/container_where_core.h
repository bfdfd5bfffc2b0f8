// Row filters in the container read's split walk (rh_k_split_where): the arithmetic of the keep words.  Free of
// HIP and shared by the kernel (container.hip) and the CPU check (tools/container_where_check.cpp), like filter_core.h.
//
// keep[] is FParams::keep's format: one word per 64 records of the FILE, bit (i & 63) of word (i >> 6) = record i is kept.  One
// lane walks one block, records first[b] .. first[b + 1] - 1 in order, so the lanes of a wavefront are at unrelated record
// indices and a word may belong to many lanes (64 one-record blocks) or a lane to many words (a 300-record block).  keep[] is
// zero at launch; a lane gathers the bits of ONE word in a register and ORs the register into memory when its next record
// lies in another word and when its block ends: at most cnt / 64 + 2 atomic ORs for a block of cnt records, none for a word in
// which the lane kept nothing.  Bits of different lanes never overlap, so the order of the ORs does not matter.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RW_HD __host__ __device__
#else
#define RW_HD
#endif

namespace rh {

struct KeepAcc {
  uint64_t word;     // index of the keep word being gathered
  uint64_t bits;     // its bits so far (only this lane's records)
};

RW_HD inline uint64_t keep_word_of(uint64_t rec) { return rec >> 6; }
RW_HD inline uint64_t keep_bit_of(uint64_t rec) { return 1ull << (rec & 63); }

// the lane's block begins at record `first`
RW_HD inline void keep_acc_init(KeepAcc& a, uint64_t first) { a.word = keep_word_of(first); a.bits = 0; }

// Record `rec` (ascending by one from `first`) with its verdict.  True = a finished word is due: OR *fbits into keep[*fword]
// (never zero bits: an empty register is dropped here).
RW_HD inline bool keep_acc_step(KeepAcc& a, uint64_t rec, bool keep, uint64_t* fword, uint64_t* fbits) {
  bool due = false;
  const uint64_t w = keep_word_of(rec);
  if (w != a.word) {
    due = a.bits != 0;
    *fword = a.word; *fbits = a.bits;
    a.word = w; a.bits = 0;
  }
  if (keep) a.bits |= keep_bit_of(rec);
  return due;
}

// The block has ended (or the lane stopped it): true = OR a.bits into keep[a.word].
RW_HD inline bool keep_acc_finish(const KeepAcc& a) { return a.bits != 0; }

// upper bound of the ORs of one block
RW_HD inline uint64_t keep_acc_max_flushes(uint64_t cnt) { return cnt / 64 + 2; }

}  // namespace rh
