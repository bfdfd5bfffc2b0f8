// Stand-alone check of a decode call's plan arithmetic (pyruhvro_amd/csrc/call_plan.h) for sanitizer builds: no HIP, no Python.
// The LDS window policy over a grid -- mean record 8 B .. 2 KB, tiles of 64 and 256 records, a fixed LDS part of 2 KB .. 120 KB,
// the generic / specialised / wide forms, the default knobs and one hand-set value of each knob -- against a table of the values
// the expressions gave while they stood inside rh_decode_call::enqueue(), and against the invariants their comments state.
// Exit status 0 = every value was the expected one.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Wall -Wextra -I pyruhvro_amd/csrc
//       tools/call_plan_check.cpp -o call_plan_check && ./call_plan_check
#include <cstdio>

#include "call_plan.h"

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { failures++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static const uint64_t kAvg[] = {8, 150, 393, 2048}, kFixed[] = {2048, 20000, 40000, 122880};
static const struct { uint64_t tile; bool specialised, wide; } kForms[] = {{256, false, false}, {256, true, false}, {64, true, false}, {64, true, true}, {64, false, true}};
static const struct { uint64_t pct, pad; long bytes; } kKnobs[] = {{115, 2048, -1}, {150, 2048, -1}, {115, 4096, -1}, {115, 2048, 16384}};
static const uint64_t kRecords = 100000;      // payload = (mean - 1) * records, as the engine's mean is payload / n + 1

// {win_bytes, big_tile_bytes}: forms x means x fixed parts x knobs, the knobs running fastest
static const uint64_t kExpected[][2] = {
    {8192, 24576}, {8192, 24576}, {8192, 24576}, {16384, 49152}, {8192, 24576}, {8192, 24576}, {8192, 24576}, {16384, 49152},
    {8192, 24576}, {8192, 24576}, {8192, 24576}, {16384, 49152}, {8192, 24576}, {8192, 24576}, {8192, 24576}, {16384, 49152},
    {46208, 138624}, {59648, 178944}, {48256, 144768}, {16384, 114321}, {46208, 138624}, {59648, 178944}, {48256, 144768}, {16384, 114321},
    {41920, 125760}, {59648, 178944}, {48256, 144768}, {16384, 114321}, {40448, 121344}, {40448, 121344}, {40448, 121344}, {16384, 114321},
    {98304, 300765}, {98304, 300765}, {98304, 300765}, {16384, 300765}, {98304, 300765}, {98304, 300765}, {98304, 300765}, {16384, 300765},
    {98304, 300765}, {98304, 300765}, {98304, 300765}, {16384, 300765}, {40448, 300765}, {40448, 300765}, {40448, 300765}, {16384, 300765},
    {98304, 1570587}, {98304, 1570587}, {98304, 1570587}, {16384, 1570587}, {98304, 1570587}, {98304, 1570587}, {98304, 1570587}, {16384, 1570587},
    {98304, 1570587}, {98304, 1570587}, {98304, 1570587}, {16384, 1570587}, {40448, 1570587}, {40448, 1570587}, {40448, 1570587}, {16384, 1570587},
    {8192, 24576}, {8192, 24576}, {8192, 24576}, {16384, 49152}, {8192, 24576}, {8192, 24576}, {8192, 24576}, {16384, 49152},
    {8192, 24576}, {8192, 24576}, {8192, 24576}, {16384, 49152}, {8192, 24576}, {8192, 24576}, {8192, 24576}, {16384, 49152},
    {38912, 116736}, {59648, 178944}, {48256, 144768}, {16384, 114321}, {20960, 114321}, {59648, 178944}, {48256, 144768}, {16384, 114321},
    {41920, 125760}, {59648, 178944}, {48256, 144768}, {16384, 114321}, {40448, 121344}, {40448, 121344}, {40448, 121344}, {16384, 114321},
    {38912, 300765}, {98304, 300765}, {98304, 300765}, {16384, 300765}, {20960, 300765}, {98304, 300765}, {98304, 300765}, {16384, 300765},
    {98304, 300765}, {98304, 300765}, {98304, 300765}, {16384, 300765}, {40448, 300765}, {40448, 300765}, {40448, 300765}, {16384, 300765},
    {38912, 1570587}, {98304, 1570587}, {98304, 1570587}, {16384, 1570587}, {20960, 1570587}, {98304, 1570587}, {98304, 1570587}, {16384, 1570587},
    {98304, 1570587}, {98304, 1570587}, {98304, 1570587}, {16384, 1570587}, {40448, 1570587}, {40448, 1570587}, {40448, 1570587}, {16384, 1570587},
    {2048, 6144}, {2048, 6144}, {2048, 6144}, {16384, 49152}, {2048, 6144}, {2048, 6144}, {2048, 6144}, {16384, 49152},
    {960, 2880}, {2048, 6144}, {2048, 6144}, {16384, 49152}, {2048, 6144}, {2048, 6144}, {2048, 6144}, {16384, 49152},
    {11552, 34656}, {14912, 44736}, {12064, 36192}, {16384, 49152}, {11552, 34656}, {14912, 44736}, {12064, 36192}, {16384, 49152},
    {11552, 34656}, {14912, 44736}, {12064, 36192}, {16384, 49152}, {11552, 34656}, {14912, 44736}, {12064, 36192}, {16384, 49152},
    {29440, 88320}, {38240, 114720}, {29952, 89856}, {16384, 75237}, {20960, 75237}, {38240, 114720}, {29952, 89856}, {16384, 75237},
    {29440, 88320}, {38240, 114720}, {29952, 89856}, {16384, 75237}, {29440, 88320}, {38240, 114720}, {29952, 89856}, {16384, 75237},
    {38912, 392898}, {98304, 392898}, {98304, 392898}, {16384, 392898}, {20960, 392898}, {98304, 392898}, {98304, 392898}, {16384, 392898},
    {98304, 392898}, {98304, 392898}, {98304, 392898}, {16384, 392898}, {40448, 392898}, {40448, 392898}, {40448, 392898}, {16384, 392898},
    {2048, 6144}, {2048, 6144}, {2048, 6144}, {16384, 49152}, {2048, 6144}, {2048, 6144}, {2048, 6144}, {16384, 49152},
    {960, 2880}, {2048, 6144}, {2048, 6144}, {16384, 49152}, {2048, 6144}, {2048, 6144}, {2048, 6144}, {16384, 49152},
    {11552, 34656}, {14912, 44736}, {12064, 36192}, {16384, 49152}, {11552, 34656}, {14912, 44736}, {12064, 36192}, {16384, 49152},
    {11552, 34656}, {14912, 44736}, {12064, 36192}, {16384, 49152}, {11552, 34656}, {14912, 44736}, {12064, 36192}, {16384, 49152},
    {18432, 75237}, {38240, 114720}, {29952, 89856}, {16384, 75237}, {29440, 88320}, {38240, 114720}, {29952, 89856}, {16384, 75237},
    {29440, 88320}, {38240, 114720}, {29952, 89856}, {16384, 75237}, {29440, 88320}, {38240, 114720}, {29952, 89856}, {16384, 75237},
    {18432, 392898}, {98304, 392898}, {98304, 392898}, {16384, 392898}, {98304, 392898}, {98304, 392898}, {98304, 392898}, {16384, 392898},
    {98304, 392898}, {98304, 392898}, {98304, 392898}, {16384, 392898}, {40448, 392898}, {40448, 392898}, {40448, 392898}, {16384, 392898},
    {2048, 6144}, {2048, 6144}, {2048, 6144}, {16384, 49152}, {2048, 6144}, {2048, 6144}, {2048, 6144}, {16384, 49152},
    {960, 2880}, {2048, 6144}, {2048, 6144}, {16384, 49152}, {2048, 6144}, {2048, 6144}, {2048, 6144}, {16384, 49152},
    {11552, 34656}, {14912, 44736}, {12064, 36192}, {16384, 49152}, {11552, 34656}, {14912, 44736}, {12064, 36192}, {16384, 49152},
    {11552, 34656}, {14912, 44736}, {12064, 36192}, {16384, 49152}, {11552, 34656}, {14912, 44736}, {12064, 36192}, {16384, 49152},
    {18432, 75237}, {38240, 114720}, {29952, 89856}, {16384, 75237}, {29440, 88320}, {38240, 114720}, {29952, 89856}, {16384, 75237},
    {29440, 88320}, {38240, 114720}, {29952, 89856}, {16384, 75237}, {29440, 88320}, {38240, 114720}, {29952, 89856}, {16384, 75237},
    {18432, 392898}, {98304, 392898}, {98304, 392898}, {16384, 392898}, {98304, 392898}, {98304, 392898}, {98304, 392898}, {16384, 392898},
    {98304, 392898}, {98304, 392898}, {98304, 392898}, {16384, 392898}, {40448, 392898}, {40448, 392898}, {40448, 392898}, {16384, 392898},
};

int main() {
  size_t i = 0, rows = 0;
  for (const auto& f : kForms)
    for (uint64_t avg : kAvg)
      for (uint64_t fixed : kFixed)
        for (const auto& kn : kKnobs) {
          rhe::WindowKnobs knobs;
          knobs.pct = kn.pct; knobs.pad = kn.pad; knobs.bytes = kn.bytes;
          const uint64_t payload = (avg - 1) * kRecords, nblocks = (kRecords + f.tile - 1) / f.tile;
          const rhe::WindowPlan w = rhe::window_plan(avg, f.tile, fixed, payload, nblocks, f.specialised, f.wide, knobs);
          EXPECT(i < sizeof kExpected / sizeof kExpected[0], "the grid is larger than the table");
          if (i < sizeof kExpected / sizeof kExpected[0])
            EXPECT(w.win_bytes == kExpected[i][0] && w.big_tile_bytes == kExpected[i][1],
                   "tile %llu spec %d wide %d mean %llu fixed %llu knobs %llu/%llu/%ld: window %u, large tile %llu; expected %llu, %llu",
                   (unsigned long long)f.tile, f.specialised, f.wide, (unsigned long long)avg, (unsigned long long)fixed, (unsigned long long)kn.pct,
                   (unsigned long long)kn.pad, kn.bytes, w.win_bytes, (unsigned long long)w.big_tile_bytes, (unsigned long long)kExpected[i][0],
                   (unsigned long long)kExpected[i][1]);
          i++;
          // the invariants: a 16-byte aligned window inside what a CDNA4 workgroup has ...
          EXPECT(w.win_bytes % 16 == 0, "window %u is not 16-byte aligned", w.win_bytes);
          EXPECT(fixed + w.win_bytes <= rhe::kLdsCap, "fixed %llu + window %u exceeds the workgroup's LDS", (unsigned long long)fixed, w.win_bytes);
          // ... and, by default on the specialised kernels of a schema that is not wide, four workgroups per CU
          const uint64_t step4 = (160 * 1024 / 4) & ~511ull;
          if (knobs.by_default() && kn.bytes < 0 && f.specialised && !f.wide && step4 > fixed + 8192)
            EXPECT(fixed + w.win_bytes <= step4, "fixed %llu + window %u leaves a CU fewer than four workgroups", (unsigned long long)fixed, w.win_bytes);
          rows++;
        }
  EXPECT(i == sizeof kExpected / sizeof kExpected[0], "the table is larger than the grid");
  // a finer sweep of the invariants alone (no table)
  size_t swept = 0;
  for (const auto& f : kForms)
    for (uint64_t avg = 8; avg <= 2048; avg += 17)
      for (uint64_t fixed = 2048; fixed <= 120 * 1024; fixed += 1808) {
        const rhe::WindowPlan w = rhe::window_plan(avg, f.tile, fixed, (avg - 1) * kRecords, (kRecords + f.tile - 1) / f.tile, f.specialised, f.wide, rhe::WindowKnobs());
        const uint64_t step4 = (160 * 1024 / 4) & ~511ull;
        EXPECT(w.win_bytes % 16 == 0 && fixed + w.win_bytes <= rhe::kLdsCap, "mean %llu fixed %llu: window %u", (unsigned long long)avg, (unsigned long long)fixed, w.win_bytes);
        if (f.specialised && !f.wide && step4 > fixed + 8192)
          EXPECT(fixed + w.win_bytes <= step4, "mean %llu fixed %llu: window %u past the four-workgroup step", (unsigned long long)avg, (unsigned long long)fixed, w.win_bytes);
        swept++;
      }
  // the explicit chunk geometry: num_chunks chunks of chunk_rows rows, the last one takes the rest (and is not empty)
  EXPECT(rhe::explicit_geometry_ok(10, 3, 4) && rhe::explicit_geometry_ok(10, 1, 4) && rhe::explicit_geometry_ok(0, 1, 4), "sound geometries refused");
  EXPECT(!rhe::explicit_geometry_ok(10, 0, 4) && !rhe::explicit_geometry_ok(10, 4, 4) && !rhe::explicit_geometry_ok(8, 3, 4) &&
         !rhe::explicit_geometry_ok(10, 1ull << 32, 4), "unsound geometries accepted");
  std::printf("call_plan_check: %zu table rows, %zu swept plans, %d failures\n", rows, swept, failures);
  return failures ? 1 : 0;
}
