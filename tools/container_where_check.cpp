// CPU check of pyruhvro_amd/csrc/container_where_core.h (the twin of filter_check.cpp and frame_check.cpp: its own main, no HIP,
// no Python).
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I pyruhvro_amd/csrc
//       tools/container_where_check.cpp -o container_where_check && ./container_where_check
//
// The keep-word accumulation of rh_k_split_where (container.hip) in the kernel's order -- workgroups of 256 lanes, wavefronts of
// 64, one lane per block, every lane of a wavefront taking its j-th record in the same round, a lane without a j-th record
// sitting the round out, the register ORed into keep[] when the lane moves on to another word and when its block ends -- against
// the plain restatement: a std::vector<bool> per record, packed in order.
//   block tables   all blocks of one record (1 .. 508 of them); cycles of ragged counts with empty blocks; one block of 1, 63, 64,
//                  65, 128, 1100 records; blocks that end exactly on a word edge and one off it; no block; only empty blocks
//   masks          none, all, alternating, first only, last only, random
//   a lane that stops its block (a malformed record): the records in front keep their bits, the rest have none
// Checked: every word, the bits behind record n - 1 (zero), the kept count, at most cnt / 64 + 2 ORs per block, no OR of an
// empty register.  keep[] and every table sit in heap blocks of exactly their size.
// Exit status 0 = no failure; the last line says what ran.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "container_where_core.h"
#include "filter_core.h"

using namespace rh;

static int failures = 0;
static size_t checks = 0, cases = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    checks++;                                             \
    if (!(cond)) {                                        \
      failures++;                                         \
      if (failures <= 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                     \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 33);
}

// One launch.  stop_block / stop_at: lane stop_block fails at its record stop_at (stop_block = ~0: nobody fails).
static void run_case(const std::string& what, const std::vector<uint64_t>& counts, const std::vector<bool>& mask, uint64_t stop_block, uint64_t stop_at) {
  cases++;
  const uint64_t nb = counts.size();
  std::unique_ptr<uint64_t[]> first(new uint64_t[nb + 1]);
  first[0] = 0;
  for (uint64_t b = 0; b < nb; b++) first[b + 1] = first[b] + counts[b];
  const uint64_t n = first[nb];
  CHECK(mask.size() == n, "%s: mask size", what.c_str());
  const uint64_t words = filter_words(n);
  std::unique_ptr<uint64_t[]> keep(new uint64_t[words]);      // (exactly ceil(n / 64) words: an OR past them is a heap overflow)
  for (uint64_t w = 0; w < words; w++) keep[w] = 0;           // the memset in front of the launch
  uint64_t kept = 0;

  const uint64_t kGroup = 256, kWave = 64;
  for (uint64_t g0 = 0; g0 < nb; g0 += kGroup) {
    for (uint64_t w0 = g0; w0 < g0 + kGroup; w0 += kWave) {
      KeepAcc acc[kWave];
      uint64_t j[kWave], flushes[kWave], nkept[kWave];
      bool stopped[kWave];
      for (uint64_t l = 0; l < kWave; l++) {
        const uint64_t b = w0 + l;
        keep_acc_init(acc[l], b < nb ? first[b] : 0);
        j[l] = 0; flushes[l] = 0; nkept[l] = 0; stopped[l] = false;
      }
      for (;;) {
        bool any = false;
        for (uint64_t l = 0; l < kWave; l++) {
          const uint64_t b = w0 + l;
          const bool mine = b < nb;
          const bool go = mine && !stopped[l] && j[l] < counts[mine ? b : 0];
          if (!go) continue;
          any = true;
          const uint64_t rec = first[b] + j[l];
          if (b == stop_block && j[l] == stop_at) { stopped[l] = true; j[l]++; continue; }      // (the malformed record: no bit)
          uint64_t fw = 0, fb = 0;
          if (keep_acc_step(acc[l], rec, mask[rec], &fw, &fb)) {
            CHECK(fb != 0, "%s: an empty register was flushed", what.c_str());
            CHECK(fw < words, "%s: flush of word %llu of %llu", what.c_str(), (unsigned long long)fw, (unsigned long long)words);
            CHECK((keep[fw] & fb) == 0, "%s: two lanes own a bit of word %llu", what.c_str(), (unsigned long long)fw);
            keep[fw] |= fb;
            flushes[l]++;
          }
          nkept[l] += mask[rec] ? 1 : 0;
          j[l]++;
        }
        if (!any) break;
      }
      for (uint64_t l = 0; l < kWave; l++) {
        const uint64_t b = w0 + l;
        if (b >= nb) continue;
        if (keep_acc_finish(acc[l])) {
          CHECK(acc[l].word < words, "%s: last flush of word %llu of %llu", what.c_str(), (unsigned long long)acc[l].word, (unsigned long long)words);
          CHECK((keep[acc[l].word] & acc[l].bits) == 0, "%s: two lanes own a bit of word %llu", what.c_str(), (unsigned long long)acc[l].word);
          keep[acc[l].word] |= acc[l].bits;
          flushes[l]++;
        }
        CHECK(flushes[l] <= keep_acc_max_flushes(counts[b]), "%s: block %llu of %llu records: %llu flushes", what.c_str(), (unsigned long long)b,
              (unsigned long long)counts[b], (unsigned long long)flushes[l]);
        kept += nkept[l];
      }
    }
  }

  // the plain restatement
  std::vector<bool> want(mask);
  if (stop_block != ~0ull)
    for (uint64_t r = first[stop_block] + stop_at; r < first[stop_block + 1]; r++) want[r] = false;
  std::vector<uint64_t> ref(words, 0);
  uint64_t ref_kept = 0;
  for (uint64_t i = 0; i < n; i++)
    if (want[i]) { ref[i >> 6] |= 1ull << (i & 63); ref_kept++; }
  for (uint64_t w = 0; w < words; w++) {
    CHECK(keep[w] == ref[w], "%s: word %llu is %016llx, not %016llx", what.c_str(), (unsigned long long)w, (unsigned long long)keep[w], (unsigned long long)ref[w]);
    CHECK((keep[w] & ~filter_valid_mask(n, w)) == 0, "%s: word %llu has bits behind record n - 1", what.c_str(), (unsigned long long)w);
  }
  CHECK(kept == ref_kept, "%s: kept %llu, not %llu", what.c_str(), (unsigned long long)kept, (unsigned long long)ref_kept);
  for (uint64_t i = 0; i < n; i++) CHECK(filter_kept(keep.get(), n, i) == (bool)want[i], "%s: record %llu", what.c_str(), (unsigned long long)i);
}

static const char* const kMaskName[] = {"none", "all", "alternating", "first", "last", "random", "random2", "random_sparse"};

static std::vector<bool> make_mask(int which, uint64_t n) {
  std::vector<bool> m(n, false);
  for (uint64_t i = 0; i < n; i++) {
    switch (which) {
      case 0: break;
      case 1: m[i] = true; break;
      case 2: m[i] = (i & 1) == 0; break;
      case 3: m[i] = i == 0; break;
      case 4: m[i] = i + 1 == n; break;
      case 5: case 6: m[i] = (rnd() & 1) != 0; break;
      default: m[i] = rnd() % 97 == 0; break;
    }
  }
  return m;
}

static void run_table(const std::string& name, const std::vector<uint64_t>& counts) {
  uint64_t n = 0;
  for (uint64_t c : counts) n += c;
  for (int which = 0; which < 8; which++) {
    const std::vector<bool> m = make_mask(which, n);
    run_case(name + " / " + kMaskName[which], counts, m, ~0ull, 0);
  }
  // a lane that stops: the fullest block, at its first, a middle and its last record
  uint64_t big = 0;
  for (uint64_t b = 0; b < counts.size(); b++)
    if (counts[b] > counts[big]) big = b;
  if (!counts.empty() && counts[big]) {
    const uint64_t at[] = {0, counts[big] / 2, counts[big] - 1};
    for (uint64_t a : at) run_case(name + " / all, block " + std::to_string(big) + " stops at " + std::to_string(a), counts, make_mask(1, n), big, a);
    run_case(name + " / random, block " + std::to_string(big) + " stops", counts, make_mask(5, n), big, counts[big] / 2);
  }
}

int main() {
  // all blocks of one record: a word belongs to 64 lanes; two workgroups
  for (uint64_t nb : {1ull, 2ull, 63ull, 64ull, 65ull, 127ull, 128ull, 129ull, 256ull, 257ull, 508ull})
    run_table("ones x " + std::to_string(nb), std::vector<uint64_t>(nb, 1));
  // ragged cycles with empty blocks: a 300-record block over five or six words beside idle lanes
  {
    std::vector<uint64_t> ragged = {0, 1, 300, 1, 0, 64, 2};
    for (uint64_t i = 0; i < 70; i++) ragged.push_back((i * 7) % 5);
    run_table("ragged", ragged);
    std::vector<uint64_t> cycle;
    for (uint64_t i = 0; i < 600; i++) cycle.push_back((i * 11) % 7 == 3 ? 0 : (i * 13) % 9);
    run_table("cycle of 600", cycle);
    std::vector<uint64_t> wide;
    for (uint64_t i = 0; i < 130; i++) wide.push_back(i % 5 == 0 ? 0 : 60 + (i * 3) % 10);
    run_table("blocks around 64", wide);
  }
  // one block: one lane owns every word
  for (uint64_t c : {1ull, 63ull, 64ull, 65ull, 128ull, 1100ull}) run_table("one block of " + std::to_string(c), {c});
  // blocks that end exactly on a word edge, and one off it
  run_table("word edges", {64, 128, 63, 65, 188});
  run_table("edges: 64 x 3", {64, 64, 64});
  run_table("edges: 63 1 64", {63, 1, 64});
  run_table("edges: 65 63", {65, 63});
  run_table("edges: 127 1 1 127", {127, 1, 1, 127});
  run_table("edges: 1 64 64 63", {1, 64, 64, 63});
  run_table("edges: 0 64 0 64 0", {0, 64, 0, 64, 0});
  run_table("edges: 192 then ones", {192, 1, 1, 1});
  // n = 0
  run_table("no block", {});
  run_table("one empty block", {0});
  run_table("only empty blocks", std::vector<uint64_t>(300, 0));

  std::printf("container_where_check: %zu launches\n", cases);
  std::printf("container_where_check: %zu checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
