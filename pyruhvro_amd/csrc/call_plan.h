// The arithmetic of one device-resident decode call's plan (engine_device_call.cpp), free of HIP so that a stand-alone host
// program can check it (tools/call_plan_check.cpp): the explicit chunk geometry, the offsets inside the control block, and the
// LDS window policy.  Pure functions of their arguments: the environment knobs are read by the caller.
#pragma once
#include <algorithm>

#include "program.h"

namespace rhe {

constexpr uint64_t kAlign = 256;
inline uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// rh_opts.chunk_rows: do the n records make num_chunks chunks of chunk_rows rows, the last one taking the rest?
inline bool explicit_geometry_ok(uint64_t n, uint64_t num_chunks, uint64_t chunk_rows) {
  return num_chunks >= 1 && num_chunks <= 0xFFFFFFFFull && (num_chunks - 1) <= n / chunk_rows &&
         !(n > 0 && n == (num_chunks - 1) * chunk_rows && num_chunks > 1);
}

// ---- control block: [first_bad u64 | layout flag, ticket | arena bytes | pad][totals u64 K*k][tickets u32 k][nullcount u32 nnodes*k*null_slots]
struct CtrlPlan {
  // o_tot: behind the control words (program.h): first_bad, layout flag, arena bytes used, pad; words 8..11 = the tile statistics
  //        (summed by rh_k_scan_layout / rh_k_tile_stats, kernels.hip)
  // o_tick: [k] tile tickets of the single-pass form (zero like the rest of the block)
  // o_flag_h: the token in the HOST layout (rh_k_publish): head | compact null counts | token
  uint64_t o_tot = 48, o_tick = 0, o_null = 0, o_flag_h = 0, bytes = 0;
  uint32_t null_slots = rh::kNullSlots;      // program.h null_slots_for(k)
};
inline CtrlPlan ctrl_plan(int K, int nnodes, uint32_t k) {
  CtrlPlan c;
  c.o_tick = c.o_tot + 8ull * K * k;
  c.o_null = align_up(c.o_tick + 4ull * k, 16);
  c.null_slots = rh::null_slots_for(k);
  c.o_flag_h = align_up(c.o_null + 4ull * nnodes * k, 8);
  // (with one null-count slot -- k > 2048 chunks -- the slot area is no larger than the compact host layout, whose publish
  //  token sits behind the summed counts: room for it, whatever the rounding)
  c.bytes = align_up(std::max<uint64_t>(c.o_null + 4ull * nnodes * k * c.null_slots, c.o_flag_h + 8), kAlign);
  return c;
}

// ---- LDS: fixed part + input window sized from the mean record length (a workgroup whose records do not fit falls back to
// global reads).  The caller refuses a schema whose fixed part leaves no 4 KB of window (lds_fixed + 4096 > kLdsCap).
constexpr uint64_t kLdsCap = 160 * 1024 - 512;
struct WindowKnobs {
  uint64_t pct = 115, pad = 2048;      // RUHVRO_HIP_WIN_PCT, RUHVRO_HIP_WIN_PAD
  long bytes = -1;         // RUHVRO_HIP_WIN_BYTES: the window as given -- 0 = none, every tile is walked from global memory; measurement knob
  bool by_default() const { return pct == 115 && pad == 2048; }      // (not when a test / sweep sets the window by hand)
};
struct WindowPlan { uint32_t win_bytes; uint64_t big_tile_bytes; };
inline WindowPlan window_plan(uint64_t avg, uint64_t tile, uint64_t lds_fixed, uint64_t payload, uint64_t nblocks, bool specialised,
                              bool wide, const WindowKnobs& kn) {
  uint64_t win = align_up(avg * tile * kn.pct / 100 + kn.pad * tile / rh::kBlock, 16);
  win = std::max<uint64_t>(win, 8192 * tile / rh::kBlock);
  win = std::min<uint64_t>(win, std::min<uint64_t>((kLdsCap - lds_fixed) & ~15ull, 96 * 1024));
  // Occupancy steps: a CU's 160 KB hold N workgroups of at most 160 KB / N each.  A window that puts the workgroup just
  // above a step costs a whole workgroup per CU (a quarter of the resident waves at N = 4) for a few hundred bytes of
  // slack, so it gives that slack up as long as a smaller margin (6 % + 1 KB over the mean tile) is left.
  if (kn.by_default()) {
    const uint64_t min_win = align_up(avg * tile * 106 / 100 + 1024 * tile / rh::kBlock, 16);
    for (uint64_t nwg = 4; nwg >= 2; nwg--) {        // (4: what the emit kernel's registers allow at most)
      const uint64_t step = (160 * 1024 / nwg) & ~511ull;
      if (lds_fixed + win > step && step > lds_fixed && step - lds_fixed >= min_win) { win = (step - lds_fixed) & ~15ull; break; }
    }
    // Round 6: never a window that leaves a CU fewer than four workgroups.  Records too large for it (a mean tile of 40 KB and
    // more: ~150 B per record) are walked in ranges by the ranged kernels, which keeps sixteen wavefronts per CU resident --
    // measured on the skewed workload (mean record 393 B): 7.1 ms with a 40 KB window, 10.7 ms with the 100 KB one the mean
    // tile asks for (profiles/r06_c_*).  Only with the specialised kernels: the generic ones have no ranges.
    if (specialised && !wide) {
      const uint64_t step4 = (160 * 1024 / 4) & ~511ull;
      if (step4 > lds_fixed + 8192 && lds_fixed + win > step4) win = (step4 - lds_fixed) & ~15ull;
    }
    // A wide schema's tile is one wavefront: the window is kept small enough for 8 of them per CU (records of a hundred and more
    // columns are large: a window for 64 of them would leave a CU one or two wavefronts) -- tiles past it are walked in ranges.
    if (wide) {
      const uint64_t per_wave = (160 * 1024 / 8) & ~511ull;
      if (per_wave > lds_fixed + 4096) win = std::min<uint64_t>(win, (per_wave - lds_fixed) & ~15ull);
    }
  }
  if (kn.bytes >= 0) win = std::min<uint64_t>((uint64_t)kn.bytes & ~15ull, (kLdsCap - lds_fixed) & ~15ull);
  // (the ranged pair takes LARGE tiles first, program.h KParams::worklist: large = well beyond both the window and this call's mean
  //  tile -- every tile of a wide schema is several windows)
  return {(uint32_t)win, (uint64_t)rh::kBigTileWindows * std::max<uint64_t>(win, nblocks ? payload / nblocks : 0)};
}

}  // namespace rhe
