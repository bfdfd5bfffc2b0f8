// One device-resident decode call: the launch sequence (k_size -> k_scan+k_layout -> k_init -> k_emit -> k_publish),
// its settlement, and the in-call split over internal streams.
#include "engine_internal.h"

using namespace rhe;

// The head of a control block handed to a pinned host block behind a token: rh_k_publish copies the head words (and the summed
// null counts), leaves the device block zeroed and stores the token last.  The host spins on that word: this call only (later
// calls stay queued behind it), no event in the stream, and sooner than a stream wait returns.  The main call and the lean
// probe both hand over this way.
struct Handover {
  void* hdev = nullptr;              // the host block as the device sees it
  volatile uint32_t* flag = nullptr;
  uint32_t token = 0;
  enum Seen { TOKEN, DONE_WITHOUT, FAILED };
  // Can a kernel write this pinned block?  (Asked before anything of the hand-over is launched: the caller keeps its fall-back.)
  bool map(uint8_t* host) {
    if (hipHostGetDevicePointer(&hdev, host, 0) == hipSuccess && hdev) return true;
    (void)hipGetLastError();
    return false;
  }
  // rh_launch_publish's status: head_words of the block at d_ctrl, null_entries summed counts behind them, the token at flag_off
  int publish(uint8_t* d_ctrl, uint8_t* host, uint32_t head_words, uint32_t null_entries, uint64_t flag_off, uint32_t null_slots, hipStream_t stream) {
    static std::atomic<uint32_t> next_token{1};      // one counter for the process; a token is never 0 (the cleared flag word)
    do token = next_token.fetch_add(1); while (token == 0);
    flag = (volatile uint32_t*)(host + flag_off);
    *flag = 0;
    return rh_launch_publish(d_ctrl, hdev, head_words, null_entries, (uint32_t)(flag_off / 4), token, null_slots, stream);
  }
  Seen wait(hipStream_t stream, hipError_t* why = nullptr) const {
    for (uint32_t spins = 0; __atomic_load_n(flag, __ATOMIC_ACQUIRE) != token;) {
      if ((++spins & 0xFFFFu) == 0) {              // a failed launch or a fault must not hang the caller
        const hipError_t q = hipStreamQuery(stream);
        // everything on the stream is done: the token is there or never will be
        if (q == hipSuccess) return __atomic_load_n(flag, __ATOMIC_ACQUIRE) == token ? TOKEN : DONE_WITHOUT;
        if (q != hipErrorNotReady) { if (why) *why = q; return FAILED; }
      }
#if defined(__x86_64__)
      __builtin_ia32_pause();
#endif
    }
    return TOKEN;
  }
};

// One device-resident decode call.  enqueue() puts the whole call on the stream (k_size -> k_scan+k_layout -> k_init ->
// k_emit -> one D2H of the control words) and finish() waits for it and settles the result (error check, arena
// retry, host tables).  rh_decode_device runs both back to back; with RH_ASYNC the result is handed out between the
// two and rh_device_result_wait() (or the first accessor that needs a host-side fact) runs finish(): the caller's next
// call is on the stream before this one has drained, which is what a pipeline of small batches needs -- a 1M-record
// call is 0.15 ms of kernels behind ~25 us of host turn-around (profiles/r03q_timeline_*.txt).
struct rh_decode_call {
  // the call
  rh_schema* s;
  const CompiledSchema& cs;
  const uint8_t* d_data;
  const uint64_t* d_offsets;
  uint64_t data_len, n, num_chunks;
  rh_opts opts;                 // by value: an asynchronous call outlives the caller's struct
  bool want_stats;
  rh_stats st;
  rh_device_result& r;
  HostProf hp;
  bool range_of_host_call = false;   // a chunk range of a host call (decode_range) or a group of a split call: the caller gave the geometry
  bool async = false;           // RH_ASYNC: the call is settled later; without rh_k_publish its end is marked with a DoneEvent
  // in-call overlap (decode_device_split, staggered form): this group's size pass starts behind `start_after` (the previous
  // group's size pass) and marks its own end with `sized`, so that size pass g+1 runs beside emit pass g
  hipEvent_t start_after = nullptr, sized = nullptr;
  // geometry (chunk_geometry; the tiles follow from the kernel form: choose_kernels)
  int device = 0;
  hipStream_t stream = nullptr;
  ChunkGeo geo_v;
  const ChunkGeo* geo = nullptr;
  uint32_t k = 1, nblocks = 0;
  int K = 0, nnodes = 0, nbuf = 0;
  const DeviceProgram* dp = nullptr;
  uint64_t narrow_rows = 0, tile = 0, bpc64 = 0, payload = 0;
  // kernel choice (choose_kernels, lean_select)
  const SpecKernel* sk = nullptr;
  hipFunction_t size_r = nullptr, emit_r = nullptr;     // the ranged pair, when this call launches it (tiles past the LDS window)
  // The pair the two-pass form launches: the schema's default (wide) rh_spec_size / rh_spec_emit, or its lean pair (lean_select)
  hipFunction_t size_f = nullptr, emit_f = nullptr;
  hipFunction_t lean_size = nullptr, lean_emit = nullptr;      // the lean pair, loaded, when this call qualifies for it
  bool lean = false;            // ... and launches it
  // control block, workspace, tables (place_blocks)
  CtrlPlan cp;
  Lease ws, hctrl, dtab, prof_buf;
  std::unique_ptr<CtrlLease> ctrl;
  rh::KParams P;
  uint64_t n_entries = 0, tab_bytes = 0;
  uint64_t* d_sizes = nullptr;
  bool child_bitmaps = false, size_pass = false;
  // window (set_window)
  uint32_t lds_bytes = 0;
  // the submission (try_single / submit_two_pass) and its settlement (finish)
  Events ev;
  std::vector<uint64_t> totals;
  uint64_t exact = 0;
  bool fused = false, timed_size = false;
  bool single = false;          // the single-pass form ran (rh_spec_fused): arena laid out from capacities
  std::vector<uint64_t> caps;   // [K][k] those capacities
  uint64_t arena_cap = 0;
  Lease lookback, hcaps;
  double basis = 0;
  bool published = false;       // rh_k_publish ran: hctrl holds the compact layout (summed null counts) behind a token
  Handover head;
  DoneEvent done;
  bool settled = false;         // finish() ran (or the call completed inside enqueue())
  // the probe (launch_probe): the lean size kernel over a sample of this call's tiles, on a workspace and control block of its own
  bool probing = false;
  Handover probe_head;
  Lease probe_ws, probe_host;
  std::unique_ptr<CtrlLease> probe_ctrl;

  rh_decode_call(rh_schema* s_, const uint8_t* data, const uint64_t* offs, uint64_t dl, uint64_t n_, uint64_t nc, const rh_opts* o,
               bool stats, const ChunkGeo* g, rh_device_result& res)
      : s(s_), cs(*s_->cs), d_data(data), d_offsets(offs), data_len(dl), n(n_), num_chunks(nc), opts(o ? *o : default_opts()),
        want_stats(stats), r(res) {
    std::memset(&st, 0, sizeof st);
    if (g) { geo_v = *g; geo = &geo_v; range_of_host_call = true; }
    opts.devices = nullptr; opts.n_devices = 0; opts.device_stats = nullptr; opts.ready = nullptr; opts.gathered = nullptr;   // (not used below; never dangling)
  }

  // Where the call's Arrow buffers go: HBM, or -- host calls, RH_INTERNAL_HOST_ARENA -- a pooled block of PINNED HOST memory that
  // the emit kernel fills through the PCIe link and that is then lent to the result (engine_export.cpp to_host_impl): no D2H
  // copy, no host wait between kernels and copy, and the copy engine is left to the H2D copies of the next chunk group (the two
  // directions on SDMA shared ~56 GB/s between them: a 1M-record call's D2H copies ran at 32 GB/s beside its H2D copies,
  // profiles/r05h_*).  The CUs' stores reach the full rate of the link: 53 GB/s, what a D2H copy of the same bytes reaches
  // (profiles/r05i_host_arena.txt).  Only with a block that sits idle in the pool -- allocating one costs 0.2 ms per MB, so the
  // pool is refilled in the background (Pool::prefetch) -- and not for schemas whose child-domain bitmaps are built with
  // atomics on the arena.  RUHVRO_HIP_HOST_ARENA=0 turns it off (A/B).
  Lease arena_lease(uint64_t bytes) {
    r.arena_host = false;
    if ((opts.flags & RH_INTERNAL_HOST_ARENA) && !child_bitmaps && env_long("RUHVRO_HIP_HOST_ARENA", 1, 0, 1) != 0) {
      Block b = pin_pool().try_get(bytes, device);
      if (b.p) {
        r.arena_host = true;
        return Lease(pin_pool(), b);
      }
      pin_pool().prefetch(bytes + bytes / 16, device, pinned_budget_left());
    }
    return Lease(dev_pool(), bytes, device);
  }

  void check_bad(const uint8_t* h) {
    unsigned long long fb = *(const unsigned long long*)h;
    if (!fb) return;
    const uint64_t rec = ~fb;
    uint64_t c = r.sz ? std::min<uint64_t>(rec / r.sz, k - 1) : 0;
    uint64_t b = c * bpc64 + (rec - c * r.sz) / tile;
    rh::ErrInfo ei;
    HIPCHK(hipMemcpy(&ei, P.errinfo + b, sizeof ei, hipMemcpyDeviceToHost));
    throw RecordDecodeError(format_error(ei));
  }

  // A call without a size pass (a schema without counters): its emit kernels counted the tiles past the window they walked
  // (control words 9 and 11: spec_flat.h, kernels.hip k_emit_body) -- the only tile statistics of such a call, and what tells the schema's
  // next calls to launch the ranged pair.  hctrl holds the head of the control block as the call's last emit pass left it.
  void learn_unsized_tiles() {
    if (timed_size || single || n == 0) return;
    const uint32_t* stw = tile_stats();
    count(RH_CTR_OVER_WINDOW_TILES, stw[1]); count(RH_CTR_SUBTILED_TILES, stw[3]);
    ranged_learn(stw[1] != 0);
  }

  // The tile statistics of the call, control words 8..11 as hctrl holds them: careful tiles, tiles past the window, re-walked
  // wavefronts, tiles walked in ranges
  const uint32_t* tile_stats() const { return (const uint32_t*)(hctrl.ptr() + 32); }

  // Tiles past the window: this schema's next kRangedKeep calls launch the ranged pair (and compile it if need be); a call that
  // met none counts that down
  void ranged_learn(bool met) {
    if (met) { s->ranged_calls.store(kRangedKeep, std::memory_order_relaxed); return; }
    uint32_t v = s->ranged_calls.load(std::memory_order_relaxed);
    if (v) s->ranged_calls.compare_exchange_weak(v, v - 1, std::memory_order_relaxed);
  }

  // program.h LParams of this call's arena layout: from the device's totals (narrow: the specialised kernels' 32-bit bounds are
  // checked) or from the single-pass form's capacities
  rh::LParams layout_params(uint64_t* col_totals, bool narrow) const {
    rh::LParams LP;
    std::memset(&LP, 0, sizeof LP);
    LP.totals = col_totals; LP.desc = dp->desc; LP.sz = r.sz; LP.rows_last = r.rows_last; LP.n = n; LP.k = k;
    LP.nbuf = nbuf; LP.K = K; LP.ndom = cs.ndom; LP.arena = r.arena.ptr(); LP.capacity = r.arena.b.size;
    LP.bufptr = (void**)dtab.ptr(); LP.bufsize = d_sizes; LP.ctrl = P.first_bad; LP.narrow = narrow ? 1u : 0u;
    LP.narrow_rows = narrow_rows;
    return LP;
  }

  // The call's last launch: the head of the control block goes to hctrl behind a token (Handover), which also leaves the block
  // zeroed for its next user -- or, where a kernel cannot write hctrl (or RUHVRO_HIP_NO_PUBLISH=1), one D2H copy of the block
  // and, for an asynchronous call, an event behind it.
  void publish_head(bool allowed) {
    if (allowed && head.map(hctrl.ptr())) {
      if (head.publish(ctrl->ptr(), hctrl.ptr(), (uint32_t)(cp.o_null / 4), (uint32_t)(nnodes * (int)k), cp.o_flag_h, cp.null_slots, stream))
        throw HipError("k_publish launch failed");
      ctrl->b.clean = true;
      published = true;
    } else {
      HIPCHK(hipMemcpyAsync(hctrl.ptr(), ctrl->ptr(), cp.bytes, hipMemcpyDeviceToHost, stream));
      if (async) done.record(device, stream);
    }
  }

  // host statement of the layout (same rule, same table order as rh_k_layout): fills the result's tables
  void layout_host() {
    r.data_bytes = totals;
    for (auto t : totals)
      if (t > 0x7FFFFFFFull) {
        count(RH_CTR_OFFSET32_ERRORS);
        throw DecodeError("offset overflow: a chunk's column exceeds the 2^31-1 limit of 32-bit Arrow offsets");
      }
    if (sk)
      for (int d = 1; d < cs.ndom; d++)
        for (uint32_t c = 0; c < k; c++)
          if (totals[(size_t)(d - 1) * k + c] >= narrow_rows) {
            if (lean) lean_count(LC_NEED_WIDE_INDEX);
            throw NeedWideIndex();
          }
    r.fill_tables();
    exact = r.output_bytes;
  }

  void launch_tail(bool offsets_done) {     // k_init + k_emit through the device tables at dtab
    if (nbuf > 0 && (child_bitmaps || !offsets_done) &&
        rh_launch_init(P.bufptr, d_sizes, dp->desc, (uint32_t)nbuf, k, P.first_bad, stream)) throw HipError("k_init launch failed");
    if (n > 0) {
      if (sk ? launch_module(emit_f, P, nblocks, (uint32_t)tile, lds_bytes, stream, ev.at(3), P.ranged ? nullptr : ev.at(4))
             : (cs.projected ? rh_launch_emit_drop : rh_launch_emit)(&P, lds_bytes, stream, ev.at(3), ev.at(4)))
        throw HipError("k_emit launch failed");
      if (P.ranged && launch_module(emit_r, P, nblocks + (P.worklist ? rh::kBigFront : 0u), (uint32_t)tile, lds_bytes, stream, nullptr, ev.at(4))) throw HipError("k_emit (ranged) launch failed");
    } else {
      ev.rec(3, stream);
      ev.rec(4, stream);
    }
  }

  void exact_tail() {      // totals are on the host: exactly sized arena, tables from the host
    ctrl->b.clean = false;
    published = false;       // (the raw device layout is copied back below)
    layout_host();
    r.arena = arena_lease(r.arena_bytes);
    Lease htab(pin_pool(), tab_bytes, device);
    void** hptr = (void**)htab.ptr();
    uint64_t* hsz = (uint64_t*)(htab.ptr() + (uint64_t)std::max(nbuf, 1) * k * 8);
    for (uint32_t c = 0; c < k; c++)
      for (int b = 0; b < nbuf; b++) {   // device tables are [chunk][buf]
        hptr[(size_t)c * nbuf + b] = r.arena.ptr() + r.buf_off[(size_t)b * k + c];
        hsz[(size_t)c * nbuf + b] = r.buf_size[(size_t)b * k + c];
      }
    HIPCHK(hipMemcpyAsync(dtab.ptr(), htab.ptr(), tab_bytes, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemsetAsync(ctrl->ptr() + 8, 0, 8, stream));    // clear the layout flag (and the ticket) of a refused optimistic attempt
    launch_tail(false);
    // (not the totals: the host has them, and rh_k_publish may have zeroed the device copy of a refused attempt)
    HIPCHK(hipMemcpyAsync(hctrl.ptr(), ctrl->ptr(), cp.o_tot, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(hctrl.ptr() + cp.o_null, ctrl->ptr() + cp.o_null, cp.bytes - cp.o_null, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));      // also keeps htab alive until the table copy is done
    check_bad(hctrl.ptr());
  }

  // ---- the lean pair (specialize.h KP_SIZE_L / KP_EMIT_L; include/ruhvro_hip.h) ----
  // Does this two-pass call qualify, and which pair does it launch?  Qualifying: AUTO or SPECIALIZED kernels, a size pass, no
  // ranged pair in the call, a schema that has a lean pair, n >= RUHVRO_HIP_LEAN_MIN_RECORDS (0 = never); RUHVRO_HIP_LEAN=0 / 1
  // = never / always.  All read per call.  The lean pair is launched only by the single-submission form, whose scan launch
  // sums the tile statistics the selection learns from (lean_learn).  A pair that is not loaded yet starts compiling in the
  // background (RUHVRO_HIP_LEAN=1 waits for it) and the call goes ahead on the wide pair.
  SpecKernel& sel() const { return const_cast<SpecKernel&>(*sk); }
  void lean_select() {
    if (!sk || !timed_size || P.ranged || sk->lean_dead || !rh::schema_has_lean(cs)) return;
    const long force = env_long("RUHVRO_HIP_LEAN", -1, 0, 1);
    const long min_n = env_long("RUHVRO_HIP_LEAN_MIN_RECORDS", 1000000, 0, 1l << 40);
    if (force == 0 || min_n == 0 || n < (uint64_t)min_n) return;
    hipFunction_t el = sk->emit_l_fn.load(std::memory_order_acquire);
    if (!el) el = spec_kernel(s, device, force == 1 ? rh::CP_BLOCKING : rh::CP_BACKGROUND, false, false, false, true).emit_l_fn.load(std::memory_order_acquire);
    if (!el) return;
    lean_emit = el;
    lean_size = sk->size_l_fn.load(std::memory_order_acquire);
    bool use = force == 1;
    if (!use) {
      std::lock_guard<std::mutex> g(s->mu);
      use = sel().lean_state == SpecKernel::LS_LEAN;
    }
    if (use && fused) {
      size_f = lean_size; emit_f = lean_emit; lean = true;
      lean_count(LC_LEAN_CALLS);
      if (opts.flags & RH_INTERNAL_TWO_PASS) lean_count(LC_TWO_PASS_REPEATS);
    }
  }

  // The probe of a qualifying call that runs on the wide pair while the schema is undecided, or wide with its wait used up: the
  // lean size kernel over the first tiles of (up to 64 of) the call's chunks -- 64 tiles and more, or all the call has -- through
  // a KParams that describes just those tiles (kernel_common.h geometry: chunk stride sz, `bpc` tiles per chunk).  It writes a
  // workspace and a control block of its own; rh_k_tile_stats sums its tile flags and rh_k_publish hands the head over.
  // Three small launches behind the call's own; counts nothing in rh_engine_counters.
  void launch_probe() {
    if (!lean_size || lean || n == 0 || env_long("RUHVRO_HIP_LEAN", -1, 0, 1) >= 0) return;
    const uint32_t kp = std::min<uint32_t>(k, 64);
    const uint32_t per = (uint32_t)std::min<uint64_t>(bpc64, (64 + kp - 1) / kp);
    const uint64_t rows_lastp = kp == k ? r.rows_last : r.sz;
    const uint32_t tiles_last = (uint32_t)std::min<uint64_t>(per, (rows_lastp + tile - 1) / tile);
    if (per == 0 || tiles_last == 0) return;
    const uint32_t pn = (kp - 1) * per + tiles_last;
    {
      std::lock_guard<std::mutex> g(s->mu);
      SpecKernel& sl = sel();
      if (sl.lean_state == SpecKernel::LS_LEAN || sl.lean_probing) return;
      if (sl.lean_state == SpecKernel::LS_WIDE && sl.lean_wait > 0) { sl.lean_wait--; return; }
      sl.lean_probing = true;
    }
    probing = true;          // (from here on drain() / probe_settle() give the schema's flag back)
    const uint64_t q_bsum = align_up(sizeof(rh::ErrInfo) * (uint64_t)pn, kAlign);
    const uint64_t q_flag = align_up(q_bsum + 4ull * std::max(K, 1) * pn, kAlign);
    const uint64_t q_lcnt = align_up(q_flag + 4ull * pn, kAlign);
    const uint64_t q_end = align_up(q_lcnt + 4ull * (uint64_t)((cs.KL + 1) / 2) * pn * tile, kAlign) + kAlign;
    probe_ws = Lease(dev_pool(), q_end, device);
    probe_host = Lease(pin_pool(), 256, device);
    probe_ctrl.reset(new CtrlLease(cp.bytes, device, stream));      // all zero; zeroed again on its way back (CtrlPool)
    if (!probe_head.map(probe_host.ptr())) {
      probe_abandon();
      return;
    }
    rh::KParams Q = P;
    Q.k = kp; Q.rows_last = rows_lastp; Q.bpc = per; Q.nblocks = pn;
    Q.ranged = 0; Q.worklist = nullptr; Q.bigmark = nullptr; Q.all_careful = 0; Q.lookback = nullptr; Q.caps = nullptr;
    Q.first_bad = (unsigned long long*)probe_ctrl->ptr();
    Q.nullcount = (uint32_t*)(probe_ctrl->ptr() + cp.o_null);
    Q.totals = (uint64_t*)(probe_ctrl->ptr() + cp.o_tot);
    Q.tickets = (uint32_t*)(probe_ctrl->ptr() + cp.o_tick);
    Q.errinfo = (rh::ErrInfo*)probe_ws.ptr();
    Q.blocksum = (uint32_t*)(probe_ws.ptr() + q_bsum);
    Q.blockbase = Q.blocksum;                              // (not read by the size kernel)
    Q.tileflag = (uint32_t*)(probe_ws.ptr() + q_flag);
    Q.lanecnt = (uint32_t*)(probe_ws.ptr() + q_lcnt);
    Q.lanecnt32 = nullptr;
    // (the probe's head: the twelve control words, no null counts, the token behind them)
    if (launch_module(lean_size, Q, pn, (uint32_t)tile, lds_bytes, stream) ||
        rh_launch_tile_stats(probe_ctrl->ptr(), Q.tileflag, pn, stream) ||
        probe_head.publish(probe_ctrl->ptr(), probe_host.ptr(), 12, 0, 48, cp.null_slots, stream))
      throw HipError("lean probe launch failed");
  }

  void probe_abandon() noexcept {      // the probe did not run (or its call is being drained): another call may probe
    if (!probing) return;
    probing = false;
    std::lock_guard<std::mutex> g(s->mu);
    sel().lean_probing = false;
  }

  // Behind the call's own wait: the probe's head (first_bad, layout flag, tile statistics) is in probe_host behind its token.
  // No malformed record, no refusal, no careful tile and no re-walked wavefront in the sample: the schema goes lean.  Anything
  // else: wide, and the next probe comes 64 qualifying calls later.
  void probe_settle() {
    if (!probing) return;
    const bool got = probe_head.wait(stream) == Handover::TOKEN;      // (a stream that ended without it, or failed: not clean)
    const uint32_t* h = (const uint32_t*)probe_host.ptr();
    const bool clean = got && h[0] == 0 && h[1] == 0 && h[2] == 0 && h[8] == 0 && h[9] == 0 && h[10] == 0;
    lean_count(LC_PROBES);
    lean_count(clean ? LC_PROBES_CLEAN : LC_PROBES_DIRTY);
    {
      std::lock_guard<std::mutex> g(s->mu);
      SpecKernel& sl = sel();
      sl.lean_probing = false;
      if (clean) sl.lean_state = SpecKernel::LS_LEAN;
      else { sl.lean_state = SpecKernel::LS_WIDE; sl.lean_wait = 64; }
    }
    probing = false;
    if (got) { probe_ws.release(); probe_host.release(); probe_ctrl.reset(); }      // (else: kept until the call is drained)
  }

  // A lean call's own tile statistics decide the schema's future: a careful tile or a re-walked wavefront (or a refusal) moves
  // it back to the wide pair for 8, 16, ... 1024 qualifying calls (as single_backoff does); a clean lean call clears the backoff.
  void lean_learn(bool dirty) {
    if (!lean) return;
    std::lock_guard<std::mutex> g(s->mu);
    SpecKernel& sl = sel();
    if (dirty) {
      if (sl.lean_state != SpecKernel::LS_WIDE) {
        sl.lean_backoff = std::min<uint32_t>(1024, std::max<uint32_t>(8, sl.lean_backoff * 2));
        sl.lean_wait = sl.lean_backoff;
        sl.lean_state = SpecKernel::LS_WIDE;
        lean_count(LC_FALLBACKS);
      }
    } else if (sl.lean_state == SpecKernel::LS_LEAN) {
      sl.lean_backoff = 0;
    }
  }

  // The single-pass form (spec_body.h spec_fused): k_layout over per-column CAPACITIES from the schema's history, then ONE
  // kernel that sizes, scans across tiles (look-back) and emits, then rh_k_publish.  Returns false when the call does not
  // qualify (no history yet, generic kernels, knobs) -- the two-pass submission follows then.
  bool try_single(bool two_sync, long ratio_hook) {
    const bool on = (opts.flags & RH_SINGLE_PASS) != 0 || env_long("RUHVRO_HIP_SINGLE_PASS", kSinglePassDefault, 0, 1) != 0;
    // (device-resident calls only: a host call is bound by the PCIe link, and its D2H copy would carry the capacity slack)
    if (!on || range_of_host_call || (opts.flags & (RH_INTERNAL_TWO_PASS | RH_TWO_PASS)) || !sk || K <= 0 || K > 64 || n == 0 || two_sync ||
        ratio_hook >= 0)
      return false;
    if (n_entries > (1u << 16)) return false;
    if (8ull * K * k > 4ull * K * nblocks) return false;      // the capacities travel in the workspace's blocksum area (below)
    // the single-pass kernel is its own code object, compiled when a call first asks for it (in the background unless the
    // caller insists on specialised kernels): until it is there the call takes the two-pass form
    hipFunction_t fused_fn = sk->fused_fn.load(std::memory_order_acquire);
    if (!fused_fn) {
      if (sk->fused_dead) return false;
      fused_fn = spec_kernel(s, device, compile_policy(opts.flags & 3, n), false, true).fused_fn.load(std::memory_order_acquire);
      if (!fused_fn) return false;
    }
    std::vector<double> per_row;
    {
      std::lock_guard<std::mutex> g(s->mu);
      if ((int)s->per_row.size() != K) return false;
      if (s->single_cooldown > 0) { s->single_cooldown--; return false; }
      per_row = s->per_row;
    }
    // capacities: what the last call needed per row, + 4 % + a pad that covers a short chunk's noise; never more than the
    // 32-bit limits the kernels index with (a column that needs more overflows its capacity -> two-pass -> the usual errors)
    // (RUHVRO_HIP_SINGLE_SLACK_PERMILLE: knob / test hook -- below 1000 the capacities are smaller than what the last call
    //  needed, which forces the LF_CAPACITY fail-over to the two-pass form)
    const double slack = (double)env_long("RUHVRO_HIP_SINGLE_SLACK_PERMILLE", 1040, 1, 4000) / 1000.0;
    caps.assign((size_t)K * k, 0);
    for (int kk = 0; kk < K; kk++)
      for (uint32_t c = 0; c < k; c++) {
        const uint64_t rows_c = c == k - 1 ? r.rows_last : r.sz;
        uint64_t cap = (uint64_t)(per_row[(size_t)kk] * (double)rows_c * slack) + (slack >= 1.0 ? 4096 : 0);
        uint64_t lim = 0x7FFFFFFFull;
        if (kk < cs.ndom - 1) lim = std::min<uint64_t>(lim, narrow_rows - 1);       // a child row domain
        caps[(size_t)kk * k + c] = std::min(cap, lim);
      }
    {   // arena bytes of that layout (the rule of fill_tables / rh_k_layout)
      uint64_t off = 0;
      for (uint32_t c = 0; c < k; c++)
        for (int b = 0; b < nbuf; b++) {
          const rh::BufDesc& d = cs.bufs[b];
          const uint64_t rows0 = c == k - 1 ? r.rows_last : r.sz;
          const uint64_t rows = d.dom == 0 ? rows0 : caps[(size_t)(d.dom - 1) * k + c];
          off += rh::buf_slot_bytes(rh::buf_bytes(d.kind, rows, d.kind == rh::BK_DATA ? caps[(size_t)d.counter * k + c] : 0, nullptr, (uint32_t)d.counter));
        }
      arena_cap = std::max<uint64_t>(off, kAlign);
    }
    count(RH_CTR_SINGLE_PASS_CALLS);
    count(RH_CTR_FUSED_CALLS);             // (a single stream submission too)
    single = true; fused = true;
    r.arena = Lease(dev_pool(), arena_cap, device);
    lookback = Lease(dev_pool(), std::max<uint64_t>(8ull * K * nblocks, kAlign), device);
    HIPCHK(hipMemsetAsync(lookback.ptr(), 0, 8ull * K * nblocks, stream));
    // the capacities go to the device behind the leading words of the workspace's blocksum area (unused on this path)
    hcaps = Lease(pin_pool(), 8ull * K * k, device);
    std::memcpy(hcaps.ptr(), caps.data(), 8ull * K * k);
    uint64_t* d_caps = (uint64_t*)P.blocksum;
    HIPCHK(hipMemcpyAsync(d_caps, hcaps.ptr(), 8ull * K * k, hipMemcpyHostToDevice, stream));
    P.lookback = (unsigned long long*)lookback.ptr();
    P.caps = d_caps;
    const rh::LParams LP = layout_params(d_caps, false);
    if (rh_launch_layout(&LP, stream)) throw HipError("k_layout launch failed");
    if (nbuf > 0 && child_bitmaps && rh_launch_init(P.bufptr, d_sizes, dp->desc, (uint32_t)nbuf, k, P.first_bad, stream))
      throw HipError("k_init launch failed");
    const uint64_t tiles_max = std::max<uint64_t>((r.sz + tile - 1) / tile, (r.rows_last + tile - 1) / tile);
    if (launch_module(fused_fn, P, (uint32_t)(tiles_max * k), (uint32_t)tile, lds_bytes, stream, ev.at(3), ev.at(4)))
      throw HipError("k_fused launch failed");
    basis = (double)payload + 64.0 * (double)n;
    publish_head(true);
    return true;
  }

  // ---- enqueue(), step by step ----
  // 1. device, stream and the chunks: k chunks of sz rows, the last one rows_last
  void chunk_geometry() {
    if (opts.device >= 0) { HIPCHK(hipSetDevice(opts.device)); device = opts.device; }
    else HIPCHK(hipGetDevice(&device));
    stream = (hipStream_t)opts.stream;
    if ((uintptr_t)d_data & 15) throw std::invalid_argument("device payload pointer must be 16-byte aligned");

    {   // the generic kernels' dynamic-LDS limit is a per-device function attribute: set it once per device
      static std::mutex lds_mu;
      static std::vector<int> lds_done;
      std::lock_guard<std::mutex> g(lds_mu);
      if (std::find(lds_done.begin(), lds_done.end(), device) == lds_done.end()) {
        if (rh_set_max_lds(160 * 1024) != 0) throw HipError("cannot raise the dynamic LDS limit of the decode kernels");
        lds_done.push_back(device);
      }
    }

    r.cs = &cs; r.device = device; r.n = n;
    if (!geo && opts.chunk_rows) {   // a range of a larger call's chunks (one process per GPU): rh_opts.chunk_rows
      if (!explicit_geometry_ok(n, num_chunks, opts.chunk_rows))
        throw std::invalid_argument("chunk_rows: the n records do not make num_chunks chunks of chunk_rows rows (the last one takes the rest)");
      geo_v.k = (uint32_t)num_chunks; geo_v.sz = opts.chunk_rows; geo_v.rows_last = n - (num_chunks - 1) * opts.chunk_rows;
      geo_v.payload_bytes = data_len;
      geo = &geo_v;
    }
    k = geo ? geo->k : rh_clamp_chunks(n, num_chunks);
    r.k = k;
    r.sz = geo ? geo->sz : n / k;
    r.rows_last = geo ? geo->rows_last : n - (uint64_t)(k - 1) * r.sz;
    payload = geo ? geo->payload_bytes : data_len;
    K = cs.K; nnodes = (int)cs.nodes.size(); nbuf = (int)cs.bufs.size();
    dp = &device_program(s, device);
  }

  // 2. kernel form: schema-specialised (compiled once per schema, cached) or the generic interpreter; with it, the tiles
  void choose_kernels() {
    const int mode = opts.flags & 3;
    // the specialised kernels address every chunk buffer with 32-bit byte offsets
    // (every chunk buffer below 4 GiB: at most max_row_bytes per row -- 16 unless the schema has a wider fixed)
    // (RUHVRO_HIP_NARROW_ROWS: test hook that lowers the bound so that small inputs take the wide-index fallback)
    narrow_rows = (uint64_t)env_long("RUHVRO_HIP_NARROW_ROWS",
                                     (long)std::min<uint64_t>(1ull << 28, (1ull << 32) / std::max<uint32_t>(cs.max_row_bytes, 16)), 1, 1l << 28);
    const bool narrow_ok = std::max(r.sz, r.rows_last) < narrow_rows;
    if (mode != RH_KERNEL_GENERIC && n > 0 && narrow_ok) {
      const SpecKernel& k0 = spec_kernel(s, device, compile_policy(mode, n));
      if (k0.ok) sk = &k0;
      else if (mode == RH_KERNEL_SPECIALIZED) throw HipError("specialised kernel unavailable: " + k0.why);
    }
    // The ranged pair behind the size / emit kernels (spec_body.h ranged_tile): while the schema's recent calls met tiles past the
    // LDS window (rh_schema::ranged_calls, fed by the call's tile statistics), or when the caller insists on the specialised
    // kernels.  A call that meets such tiles without it is refused by its size kernel (LF_NEED_RANGED) and repeated on the generic
    // kernels (NeedRanged); a schema without counters has no size pass, so its emit kernel walks such tiles itself, carefully and
    // from global memory, and counts them (spec_flat.h; learn_unsized_tiles).  Either way the schema's next calls launch the pair, compiled
    // in the background if need be.  RUHVRO_HIP_RANGED=0 / 1: never / always (A/B, tests).
    if (sk) {
      const long force = env_long("RUHVRO_HIP_RANGED", -1, 0, 1);
      const bool want = force == 1 || (force != 0 && (s->ranged_calls.load(std::memory_order_relaxed) > 0 || mode == RH_KERNEL_SPECIALIZED));
      if (want && !sk->ranged_dead) {
        hipFunction_t er = sk->emit_r_fn.load(std::memory_order_acquire);
        // (asked for by the schema's history: never wait for the compile -- the generic kernels take the call meanwhile)
        if (!er) er = spec_kernel(s, device, (force == 1 || mode == RH_KERNEL_SPECIALIZED) ? rh::CP_BLOCKING : rh::CP_BACKGROUND, false, false, true).emit_r_fn.load(std::memory_order_acquire);
        if (er) { emit_r = er; size_r = sk->size_r_fn.load(std::memory_order_acquire); }
      }
      if (want && !emit_r) {
        if (mode == RH_KERNEL_SPECIALIZED) throw HipError("specialised kernels for tiles past the LDS window unavailable");
        sk = nullptr;            // tiles past the window are expected and the pair is not there (yet): the generic kernels
      }
    }
    // records per workgroup: a wide schema's tile is one wavefront on both kernel forms (program.h kWideTile)
    tile = cs.wide ? (uint64_t)rh::kWideTile : sk ? (uint64_t)rh::spec_tile_records() : (uint64_t)rh::kBlock;
    bpc64 = std::max<uint64_t>((r.sz + tile - 1) / tile, 1);
    const uint64_t nblocks64 = n == 0 ? 0 : (uint64_t)(k - 1) * bpc64 + (r.rows_last + tile - 1) / tile;
    if (nblocks64 > 0x7FFFFFFFull / std::max(K, 1)) throw std::invalid_argument("too many records for one call");
    nblocks = (uint32_t)nblocks64;
  }

  // 3. the control block (zeroed, CtrlPool; laid out by call_plan.h ctrl_plan), the workspace and the buffer tables; KParams over them
  void place_blocks() {
    const bool ranged = size_r && emit_r;
    cp = ctrl_plan(K, nnodes, k);
    // workspace (needs no zeroing): errinfo | blocksum | blockbase | tileflag | lanecnt
    const uint64_t o_bsum = align_up(sizeof(rh::ErrInfo) * (uint64_t)nblocks, kAlign);
    const uint64_t o_bbase = align_up(o_bsum + 4ull * K * nblocks, kAlign);
    const uint64_t o_flag = align_up(o_bbase + 4ull * K * nblocks, kAlign);
    const uint64_t o_lcnt = align_up(o_flag + 4ull * nblocks, kAlign);
    // (per-record counters from the size pass to the emit pass: two per dword for the specialised kernels, one for the generic ones)
    const uint64_t o_lcnt32 = align_up(o_lcnt + 4ull * (sk ? (uint64_t)((cs.KL + 1) / 2) : (uint64_t)cs.KL) * nblocks * tile, kAlign);
    const uint64_t o_wl = align_up(o_lcnt32 + (ranged ? 4ull * (uint64_t)cs.KL * nblocks * tile : 0), kAlign);      // (+ the ranged pair's 32-bit counters)
    const uint64_t ws_bytes = align_up(o_wl + (ranged ? 8ull + 8ull * nblocks : 0), kAlign);                           // (+ its work list: large tiles first)
    hp.mark("setup");
    ws = Lease(dev_pool(), ws_bytes, device);
    hctrl = Lease(pin_pool(), cp.bytes, device);
    ctrl.reset(new CtrlLease(cp.bytes, device, stream));        // all zero (CtrlPool)
    // the buffer tables [chunk][buf]: pointers, then sizes -- written by the layout kernel, or by the host (exact_tail)
    n_entries = (uint64_t)k * std::max(nbuf, 0);
    tab_bytes = align_up((uint64_t)std::max(nbuf, 1) * k * 16, kAlign);
    dtab = Lease(dev_pool(), tab_bytes, device);
    d_sizes = (uint64_t*)(dtab.ptr() + (uint64_t)std::max(nbuf, 1) * k * 8);
    hp.mark("leases");

    std::memset(&P, 0, sizeof P);
    P.data = d_data; P.offsets = d_offsets; P.data_len = data_len;
    P.n = n; P.sz = r.sz; P.rows_last = r.rows_last; P.k = k; P.bpc = (uint32_t)bpc64; P.nblocks = nblocks;
    P.prog = dp->prog; P.sym_off = dp->sym_off; P.sym_data = dp->sym_data;
    P.nops = (int)cs.prog.size(); P.K = K; P.KL = cs.KL; P.tile = (uint32_t)tile; P.ndom = cs.ndom; P.nnodes = nnodes; P.list_depth = cs.list_depth;
    P.nbuf = nbuf; P.cnt_databuf = dp->cnt_databuf;
    P.ranged = ranged ? 1u : 0u;
    P.first_bad = (unsigned long long*)ctrl->ptr();
    P.nullcount = (uint32_t*)(ctrl->ptr() + cp.o_null);
    P.null_slots = cp.null_slots;
    P.totals = (uint64_t*)(ctrl->ptr() + cp.o_tot);
    P.tickets = (uint32_t*)(ctrl->ptr() + cp.o_tick);
    P.errinfo = (rh::ErrInfo*)ws.ptr();
    P.blocksum = (uint32_t*)(ws.ptr() + o_bsum);
    P.blockbase = (uint32_t*)(ws.ptr() + o_bbase);
    P.tileflag = (uint32_t*)(ws.ptr() + o_flag);
    P.lanecnt = (uint32_t*)(ws.ptr() + o_lcnt);
    P.lanecnt32 = (uint32_t*)(ws.ptr() + o_lcnt32);
    P.bufptr = (void* const*)dtab.ptr();
    // (a projection without variable-length output that dropped variable-length fields keeps its size pass: schema.h size_always)
    size_pass = K > 0 || cs.size_always;
    P.worklist = (ranged && size_pass && n > 0) ? (uint32_t*)(ws.ptr() + o_wl) : nullptr;      // (filled by the size kernel: only with a size pass)
    P.bigmark = P.worklist ? P.worklist + 2 + nblocks : nullptr;
    for (const rh::BufDesc& d : cs.bufs) child_bitmaps = child_bitmaps || (d.kind == rh::BK_BITMAP && d.dom != 0);   // built with atomics on zeroed words
  }

  // 4. LDS: the kernels' fixed part + the input window (call_plan.h window_plan; its knobs are read per call)
  void set_window() {
    const uint32_t lds_fixed = (sk ? rh::spec_lds_fixed_words_host(K, nnodes, (int)(tile / 64), rh::child_bitmap_count(cs), rh::dense_list_count(cs), rh::dom0_bitmap_count(cs)) * 4 : rh_lds_fixed_bytes(K, cs.KL, (int)tile, cs.list_depth, nnodes, nbuf)) + 16;   // + window slack
    if (lds_fixed + 4096 > kLdsCap) throw rh::SchemaError("schema needs more LDS than a CDNA4 workgroup has");
    WindowKnobs kn;      // (tuning / test knobs)
    kn.pct = (uint64_t)env_long("RUHVRO_HIP_WIN_PCT", 115, 100, 400);
    kn.pad = (uint64_t)env_long("RUHVRO_HIP_WIN_PAD", 2048, 0, 65536);
    kn.bytes = env_long("RUHVRO_HIP_WIN_BYTES", -1, 0, 150 * 1024);
    const WindowPlan w = window_plan(n ? payload / n + 1 : 16, tile, lds_fixed, payload, nblocks, sk != nullptr, cs.wide, kn);
    P.win_bytes = w.win_bytes;
    P.big_tile_bytes = w.big_tile_bytes;
    lds_bytes = lds_fixed + w.win_bytes;
  }

  // 5. the two-pass form.  With a size history for this schema (`ratio`) the whole call is ONE stream submission:
  //   k_size -> k_scan -> k_layout (exact arena layout on the device, program.h LParams) -> k_init -> k_emit -> k_publish.
  // The arena is reserved up front from the history; when it turns out too small (the data changed character), the layout
  // kernel says so, init/emit return at once, and the host re-runs the tail with an exactly sized arena -- which is also what
  // the first call of a schema does (finish: exact_tail).
  // stage timings (rh_stats) come from the kernels' own start / stop timestamps: e0..e1 = k_size, e5..e2 = k_scan, e3..e4 = k_emit
  void submit_two_pass(double ratio) {
    timed_size = n > 0 && size_pass;
    size_f = sk ? sk->size_fn : nullptr;
    emit_f = sk ? sk->emit_fn : nullptr;
    lean_select();
    if (timed_size) {
      if (P.worklist) HIPCHK(hipMemsetAsync(P.worklist, 0, 8ull + 8ull * nblocks, stream));      // the list's length, every tile's mark

      // (with the ranged pair: the size kernel's start and the ranged size kernel's stop bracket the pass)
      if (sk ? launch_module(size_f, P, nblocks, (uint32_t)tile, lds_bytes, stream, ev.at(0), P.ranged ? nullptr : ev.at(1))
             : (cs.projected ? rh_launch_size_drop : rh_launch_size)(&P, lds_bytes, stream, ev.at(0), ev.at(1)))
        throw HipError("k_size launch failed");
      if (P.ranged && launch_module(size_r, P, nblocks + (P.worklist ? rh::kBigFront : 0u), (uint32_t)tile, lds_bytes, stream, nullptr, ev.at(1))) throw HipError("k_size (ranged) launch failed");
      if (sized) HIPCHK(hipEventRecord(sized, stream));
      // (the single-submission path scans and lays the arena out in ONE launch, below)
      if (K == 0) {      // nothing to scan; the emit kernels of a schema without counters do not read the tile flags: all carefully
        P.all_careful = 1;
        ev.rec(5, stream);
        ev.rec(2, stream);
      } else if (!fused && rh_launch_scan(&P, stream, ev.at(5), ev.at(2))) throw HipError("k_scan launch failed");
    } else {
      // no size pass (no variable-length output): nobody classified the tiles, so the emit kernel walks all of them carefully --
      // those past the window too, which it counts (kAcNoSizePass: spec_flat.h, kernels.hip k_emit_body)
      P.all_careful = 1u | kAcNoSizePass;
      if (sized) HIPCHK(hipEventRecord(sized, stream));
    }
    // RUHVRO_HIP_NO_TRUST=1 (debugging aid): the emit pass walks EVERY tile with its own bounds and anomaly checks instead of
    // trusting the size pass's verdict on the same bytes (walk.h RH_TRUST) -- what a caller that suspects its input buffers
    // change between the two passes of an RH_ASYNC call turns on; the GPU suite passes with it (tests/test_async_device.py)
    static const bool no_trust = env_long("RUHVRO_HIP_NO_TRUST", 0, 0, 1) != 0;
    if (no_trust) P.all_careful |= 1u;
    hp.mark("size+scan_launch");
    basis = (double)payload + 64.0 * (double)n;
    if (fused) {
      count(RH_CTR_FUSED_CALLS);
      const uint64_t capacity = align_up((uint64_t)(ratio * basis * 1.125) + n_entries * kAlign + (1u << 20), kAlign);
      r.arena = arena_lease(capacity);
      const rh::LParams LP = layout_params(P.totals, sk != nullptr);
      // (the tile statistics are summed by the scan launch; a size pass with nothing to scan gets a small launch of its own)
      if (timed_size && K == 0 && rh_launch_tile_stats(ctrl->ptr(), P.tileflag, nblocks, stream)) throw HipError("k_tile_stats launch failed");
      if ((timed_size && K > 0) ? rh_launch_scan_layout(&P, &LP, stream, ev.at(5), ev.at(2)) : rh_launch_layout(&LP, stream))
        throw HipError("k_scan / k_layout launch failed");
      launch_tail(true);                           // the layout kernel wrote offsets[0] = 0 itself
      hp.mark("layout+emit_launch");
      static const bool no_publish = env_long("RUHVRO_HIP_NO_PUBLISH", 0, 0, 1) != 0;
      publish_head(!no_publish);
      hp.mark("d2h_enqueue");
    }
    launch_probe();
  }

  void enqueue() {
    Range rk("ruhvro_hip:decode_device (k_size, k_scan, k_layout, k_init, k_emit)");
    chunk_geometry();
    choose_kernels();
    place_blocks();
    set_window();
    // optional in-kernel phase timing of the specialised kernels (RUHVRO_HIP_PROFILE=1)
    static const bool profile_env = [] { const char* e = std::getenv("RUHVRO_HIP_PROFILE"); return e && *e && *e != '0'; }();
    if (profile_env && sk) {
      prof_buf = Lease(dev_pool(), 64 * 32 * 8, device);
      HIPCHK(hipMemsetAsync(prof_buf.ptr(), 0, 64 * 32 * 8, stream));
      P.prof = (unsigned long long*)prof_buf.ptr();
    }
    if (want_stats) ev.init();
    hp.mark("events");

    totals.assign((size_t)K * k, 0);
    const bool two_sync = env_long("RUHVRO_HIP_TWO_SYNC", 0, 0, 1) != 0;
    // (RUHVRO_HIP_ARENA_PERMILLE: test hook, the arena is reserved as if the schema's history said that many output
    //  bytes per 1000 input bytes -- a small value forces the LF_CAPACITY retry)
    const long ratio_hook = env_long("RUHVRO_HIP_ARENA_PERMILLE", -1, 0, 1000000);
    const double ratio = ratio_hook >= 0 ? std::max(1e-9, ratio_hook / 1000.0) : s->arena_ratio.load();
    fused = n > 0 && ratio > 0 && !two_sync && n_entries <= (1u << 16);
    if (start_after) HIPCHK(hipStreamWaitEvent(stream, start_after, 0));
    if (!try_single(two_sync, ratio_hook)) submit_two_pass(ratio);
  }

  void finish() {
    if (settled) return;
    settled = true;
    HIPCHK(hipSetDevice(device));
    if (fused) {
      if (published) {
        hipError_t q = hipSuccess;
        const Handover::Seen seen = head.wait(stream, &q);
        if (seen == Handover::DONE_WITHOUT) throw HipError("rh_k_publish finished without publishing its token");
        if (seen == Handover::FAILED) throw HipError(std::string("stream failed while waiting for a decode call: ") + hipGetErrorString(q));
      } else if (done.e) {
        done.wait();                               // this call only: later calls stay queued behind it
      } else {
        HIPCHK(hipStreamSynchronize(stream));
      }
      hp.mark("sync");
      probe_settle();
      const uint32_t lflag = *(const uint32_t*)(hctrl.ptr() + 8);
      // a tile past the LDS window and no ranged pair in this call: nothing was emitted.  The refused attempt counts nothing
      // (its tiles past the window never wrote their flag words, and the device summed none): the repeat of the call does.
      // Ahead of the error check: a refused tile was not walked, so first_bad is the lowest malformed record of the OTHER tiles
      // only -- the repeat walks every tile and reports the lowest of all.
      if (lflag & rh::LF_NEED_RANGED) {
        ctrl->b.clean = published;
        ranged_learn(true);
        r.arena.release();
        if (lean) { lean_count(LC_NEED_RANGED); lean_learn(true); }
        throw NeedRanged();
      }
      check_bad(hctrl.ptr());
      // (a lean call reads its statistics whichever way the head came back: the scan launch summed them into the control block)
      const uint32_t* stw = tile_stats();
      if (lean && !single) lean_learn(stw[0] != 0 || stw[2] != 0);
      if (published && timed_size && !single) {      // the tile statistics the scan launch summed (include/ruhvro_hip.h RH_CTR_*_TILES)
        count(RH_CTR_TILES, nblocks);
        count(RH_CTR_CAREFUL_TILES, stw[0]); count(RH_CTR_OVER_WINDOW_TILES, stw[1]);
        count(RH_CTR_REWALKED_WAVES, stw[2]); count(RH_CTR_SUBTILED_TILES, stw[3]);
        ranged_learn(stw[1] != 0);
      }
      if (K > 0) std::memcpy(totals.data(), hctrl.ptr() + cp.o_tot, 8ull * K * k);
      if (single) {
        ctrl->b.clean = published;
        if (lflag) {            // a column outgrew its capacity (or the capacity layout was refused): the two-pass path decides
          // (not latched when the capacities were shrunk by the test hook)
          if ((lflag & rh::LF_CAPACITY) && env_long("RUHVRO_HIP_SINGLE_SLACK_PERMILLE", 1040, 1, 4000) >= 1000) {
            std::lock_guard<std::mutex> g(s->mu);
            s->single_backoff = std::min<uint32_t>(1024, std::max<uint32_t>(8, s->single_backoff * 2));
            s->single_cooldown = s->single_backoff;
          }
          count(RH_CTR_SINGLE_PASS_FAILOVERS);
          r.arena.release();
          throw NeedTwoPass();
        }
        r.data_bytes = totals;
        r.layout_bytes = caps;
        r.arena_bytes = arena_cap;
        { std::lock_guard<std::mutex> g(s->mu); s->single_backoff = 0; }
      } else if (lflag & rh::LF_CAPACITY) {
        count(RH_CTR_CAPACITY_RETRIES);
        if (lean) lean_count(LC_CAPACITY_TAILS);
        r.arena.release();
        exact_tail();                              // (throws the offset-overflow / wide-index cases itself)
      } else if (lflag || want_stats) {
        layout_host();                             // throws for LF_OFFSET32 / LF_NEED_WIDE: same tests on the same totals
        if (lflag) throw HipError("internal error: layout kernel and host disagree");
        if (r.arena_bytes != std::max<uint64_t>(*(const uint64_t*)(hctrl.ptr() + 16), kAlign)) throw HipError("internal error: device and host arena layouts differ");
      } else {
        // the device laid the arena out and accepted it: the host's tables (same rule, same totals) wait for their first
        // reader (rh_device_result::tables) -- a caller that only hands the device buffers on never pays for them
        r.data_bytes = totals;
        r.arena_bytes = std::max<uint64_t>(*(const uint64_t*)(hctrl.ptr() + 16), kAlign);
      }
    } else {
      count(RH_CTR_TWO_SYNC_CALLS);      // (this path counts no tile statistics: rh_k_scan sums none)
      if (timed_size) {
        HIPCHK(hipMemcpyAsync(hctrl.ptr(), ctrl->ptr(), cp.bytes, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        probe_settle();
        if (*(const uint32_t*)(hctrl.ptr() + 8) & rh::LF_NEED_RANGED) {      // (ahead of the error check, as above)
          ctrl->b.clean = false;
          ranged_learn(true);
          throw NeedRanged();
        }
        check_bad(hctrl.ptr());
        std::memcpy(totals.data(), hctrl.ptr() + cp.o_tot, 8ull * K * k);
      }
      exact_tail();
    }
    learn_unsized_tiles();
    if (n > 0 && basis > 0 && !single) {
      const double slots = (double)n_entries * (double)kAlign;
      s->arena_ratio.store(std::max(0.0, (double)r.arena_bytes - slots) / basis + 1e-9);
    }
    if (n > 0 && K > 0 && (int)totals.size() == K * (int)k) {       // per-row need of every counter's column (single-pass capacities)
      std::vector<double> pr((size_t)K, 0.0);
      for (int kk = 0; kk < K; kk++)
        for (uint32_t c = 0; c < k; c++) {
          const uint64_t rows_c = c == k - 1 ? r.rows_last : r.sz;
          if (rows_c) pr[(size_t)kk] = std::max(pr[(size_t)kk], (double)totals[(size_t)kk * k + c] / (double)rows_c);
        }
      std::lock_guard<std::mutex> g(s->mu);
      s->per_row = std::move(pr);
    }
    r.nullcount.assign((size_t)nnodes * k, 0);
    if (published) {           // rh_k_publish summed the slots: one word per (node, chunk)
      std::memcpy(r.nullcount.data(), hctrl.ptr() + cp.o_null, 4ull * nnodes * k);
    } else {
      const uint32_t* slots = (const uint32_t*)(hctrl.ptr() + cp.o_null);      // [nnodes][k][null_slots] (program.h)
      for (size_t e = 0; e < (size_t)nnodes * k; e++) {
        uint32_t sum = 0;
        for (uint32_t sl = 0; sl < cp.null_slots; sl++) sum += slots[e * cp.null_slots + sl];
        r.nullcount[e] = sum;
      }
    }
    hp.mark("host_layout");

    if (prof_buf.ptr()) {
      unsigned long long hr[64 * 32], h[32] = {0};
      HIPCHK(hipMemcpy(hr, prof_buf.ptr(), sizeof hr, hipMemcpyDeviceToHost));
      for (int r0 = 0; r0 < 64; r0++)
        for (int i = 0; i < 32; i++) h[i] += hr[r0 * 32 + i];
      const double waves = (double)nblocks * 4;
      static const char* names2[] = {"offsets", "stage+barrier", "lane_init", "walk1", "scan", "barrier", "layout", "walk2",
                                     "errors+barrier", "flush"};
      static const char* names1[] = {"ticket+zero+barrier", "offsets+stage+barrier", "size_walk", "wave_scan", "barrier", "lookback(wave0)",
                                     "barrier", "prefix", "emit_walk", "errors+flush"};
      const char* const* names = single ? names1 : names2;
      std::fprintf(stderr, "[ruhvro_hip profile] %s cycles/wave:", single ? "single-pass" : "emit");
      for (int i = 0; i < 10; i++) std::fprintf(stderr, " %s=%.0f", names[i], h[i] / waves);
      std::fprintf(stderr, "\n[ruhvro_hip profile] size cycles/wave: stage+barrier=%.0f init=%.0f walk=%.0f tail=%.0f | kernels ms: size=%.3f emit=%.3f\n",
                   h[16] / waves, h[17] / waves, h[18] / waves, h[19] / waves, ev.ms(0, 1), ev.ms(3, 4));
    }
    if (want_stats) {
      st.records = n;
      st.input_bytes = payload;
      st.output_bytes = exact;
      st.chunks = k;
      st.blocks = nblocks;
      st.size_kernel_ms = (timed_size && !single) ? ev.ms(0, 1) : 0.f;
      st.scan_kernel_ms = (timed_size && !single) ? ev.ms(5, 2) : 0.f;
      st.emit_kernel_ms = n > 0 ? ev.ms(3, 4) : 0.f;
      st.specialized = sk ? 1 : 0;
      st.lds_bytes = n > 0 ? lds_bytes : 0;      // (of the emit launch: a call without records launches none)
    }
    // the call's scratch goes back to the pools now (the control block is zeroed on its stream, CtrlPool)
    ws.release(); dtab.release(); hctrl.release(); prof_buf.release(); lookback.release(); hcaps.release(); ctrl.reset();
    probe_settle();      // (a path that waited for the stream some other way: by now the probe is done too)
  }

  // a call that failed (or is abandoned) must not hand its blocks back while the GPU may still be using them
  void drain() noexcept {
    if (stream || device >= 0) { (void)hipSetDevice(device); (void)hipStreamSynchronize(stream); }
    probe_abandon();
  }
};

rh_device_result::rh_device_result() { std::memset(&st, 0, sizeof st); }
rh_device_result::~rh_device_result() {
  if (pending) {                 // freed without a wait: the GPU may still be writing into the blocks this result owns
    pending->drain();
    pending.reset();
  }
  parts.clear();                 // (each group drains its own stream)
  if (!join_events.empty()) {
    std::lock_guard<std::mutex> g(DoneEvent::mu());
    auto& v = DoneEvent::idle()[device];
    for (hipEvent_t e : join_events) {
      if (v.size() < 64) v.push_back(e);
      else (void)hipEventDestroy(e);
    }
  }
}


namespace rhe {

typedef rh_decode_call DeviceDecode;

rh_device_result* decode_device_impl1(rh_schema* s, const uint8_t* d_data, const uint64_t* d_offsets, uint64_t data_len,
                                      uint64_t n, uint64_t num_chunks, const rh_opts* opts, rh_stats* stats, const ChunkGeo* geo) {
  auto res = std::make_unique<rh_device_result>();
  auto call = std::make_unique<DeviceDecode>(s, d_data, d_offsets, data_len, n, num_chunks, opts, stats != nullptr, geo, *res);
  const bool async = opts && (opts->flags & RH_ASYNC) && !geo;
  call->async = async;
  try {
    call->enqueue();
    if (async && call->fused) {            // everything is on the stream: settle later (rh_device_result_wait)
      if (call->lean) lean_count(LC_ASYNC_SETTLED);
      res->pending = std::move(call);
      return res.release();
    }
    call->finish();
  } catch (...) {
    call->drain();
    throw;
  }
  if (stats) {
    const float pack = stats->pack_ms, h2d = stats->h2d_ms, d2h = stats->d2h_ms, tot = stats->total_ms;
    *stats = call->st;
    stats->pack_ms = pack; stats->h2d_ms = h2d; stats->d2h_ms = d2h; stats->total_ms = tot;
  }
  return res.release();
}


// ---------------------------------------------------------------------------
// In-call overlap: a large device-resident call deals its chunk GROUPS to internal streams.
//
// The reference runs one task per chunk (ruhvro/src/deserialize.rs:92-120); chunks are independent here too, and the two
// passes load different parts of a CU (the size pass is bound by VALU issue, the emit pass co-limited by the vector-memory
// path), so the size pass of one group running beside the emit pass of another fills issue slots that either kernel
// alone leaves empty (bench.py `overlapped` measured it between independent calls; this is the same inside ONE call).
// Group g = chunks [k*g/G, k*(g+1)/G) is a complete sub-call (size -> scan+layout -> emit -> publish, its own arena and
// control block) on its own stream; the caller's stream forks into the internal streams at the start of the call and
// joins them at its end, so the result is valid in stream order on rh_opts.stream exactly like an unsplit call's.
// Not taken when the caller asks for stage timings (kernels that share the chip have no per-kernel duration), on a
// schema's first call (no size history), for the generic kernels, or below RUHVRO_HIP_SPLIT_MIN records.
// RUHVRO_HIP_INTERNAL_STREAMS=G (1 = off) -- profiler passes run with 1.
// ---------------------------------------------------------------------------
void settle(rh_device_result* r);

hipEvent_t pooled_event(int device) {
  hipEvent_t e = nullptr;
  {
    std::lock_guard<std::mutex> g(DoneEvent::mu());
    auto& v = DoneEvent::idle()[device];
    if (!v.empty()) { e = v.back(); v.pop_back(); }
  }
  if (!e) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return e;
}

// The internal streams of the in-call split on one device: created on first use, kept for the process, shared by every caller
// stream of that device (a split call forks into them from its own stream with an event and joins them back the same way, so
// they carry no caller's identity -- keyed by the caller's handle, as they were, a destroyed and re-created stream found stale
// companions and the 65th caller silently lost the split).  Calls that split at the same time on one device
// share them in stream order.
std::vector<hipStream_t> companion_streams(int device, hipStream_t /*caller*/, unsigned want) {
  static std::mutex mu;
  static std::map<int, std::vector<hipStream_t>> all;
  std::lock_guard<std::mutex> g(mu);
  auto& v = all[device];
  while (v.size() < want) {
    hipStream_t x = nullptr;
    HIPCHK(hipStreamCreateWithFlags(&x, hipStreamNonBlocking));
    v.push_back(x);
  }
  return std::vector<hipStream_t>(v.begin(), v.begin() + want);
}

rh_device_result* decode_device_split(rh_schema* s, const uint8_t* d_data, const uint64_t* d_offsets, uint64_t data_len, uint64_t n,
                                      const rh_opts& opts, uint32_t k, uint64_t sz, uint64_t rows_last, unsigned NS) {
  int device = opts.device;
  if (device >= 0) HIPCHK(hipSetDevice(device));
  else HIPCHK(hipGetDevice(&device));
  hipStream_t caller = (hipStream_t)opts.stream;
  const std::vector<hipStream_t> extra = companion_streams(device, caller, NS - 1);
  if (extra.size() != NS - 1) return nullptr;
  // groups: G >= NS runs of whole chunks, dealt to the NS streams round-robin (RUHVRO_HIP_SPLIT_GROUPS, default = NS);
  // staggered (RUHVRO_HIP_SPLIT_STAGGER, default on): group g + 1's size pass starts when group g's has finished, so it
  // runs beside group g's EMIT pass (different bounds) instead of beside its size pass (the same bound)
  const unsigned G = (unsigned)std::min<uint64_t>(k, (uint64_t)std::max<long>(env_long("RUHVRO_HIP_SPLIT_GROUPS", 0, 0, 64), (long)NS));
  const bool stagger = env_long("RUHVRO_HIP_SPLIT_STAGGER", 1, 0, 1) != 0;
  hipEvent_t prev_sized = nullptr;
  auto parent = std::make_unique<rh_device_result>();
  parent->cs = s->cs.get(); parent->device = device; parent->n = n; parent->k = k; parent->sz = sz; parent->rows_last = rows_last;
  const bool async = (opts.flags & RH_ASYNC) != 0;
  count(RH_CTR_SPLIT_CALLS);
  // fork: the internal streams start behind everything that is on the caller's stream now (the input buffers' producers)
  hipEvent_t fork = pooled_event(device);
  parent->join_events.push_back(fork);
  HIPCHK(hipEventRecord(fork, caller));
  for (hipStream_t x : extra) HIPCHK(hipStreamWaitEvent(x, fork, 0));
  for (unsigned g = 0; g < G; g++) {
    const uint32_t c0 = (uint32_t)((uint64_t)k * g / G), c1 = (uint32_t)((uint64_t)k * (g + 1) / G);
    const uint64_t r0 = (uint64_t)c0 * sz, r1 = c1 == k ? n : (uint64_t)c1 * sz;
    ChunkGeo geo;
    geo.k = c1 - c0; geo.sz = sz; geo.rows_last = c1 == k ? rows_last : sz;
    geo.payload_bytes = n ? (uint64_t)((double)data_len * (double)(r1 - r0) / (double)n) : 0;   // (the offsets live on the device)
    rh_opts o = opts;
    o.stream = g % NS == 0 ? (void*)caller : (void*)extra[g % NS - 1];
    o.device = device; o.chunk_rows = 0; o.flags &= ~RH_ASYNC;
    auto res = std::make_unique<rh_device_result>();
    auto call = std::make_unique<DeviceDecode>(s, d_data, d_offsets + r0, data_len, r1 - r0, (uint64_t)geo.k, &o, false, &geo, *res);
    call->async = true;
    if (stagger) {
      call->start_after = prev_sized;
      if (g + 1 < G) {
        prev_sized = pooled_event(device);
        parent->join_events.push_back(prev_sized);
        call->sized = prev_sized;
      }
    }
    try {
      call->enqueue();
      if (call->fused) {
        res->pending = std::move(call);
      } else {
        call->finish();
      }
    } catch (...) {
      call->drain();
      throw;                      // (the groups already enqueued drain in the parent's destructor)
    }
    parent->part_chunk0.push_back(c0);
    parent->parts.push_back(std::move(res));
  }
  // join: the caller's stream continues behind every group
  for (hipStream_t x : extra) {
    hipEvent_t e = pooled_event(device);
    parent->join_events.push_back(e);
    HIPCHK(hipEventRecord(e, x));
    HIPCHK(hipStreamWaitEvent(caller, e, 0));
  }
  if (!async) settle(parent.get());
  return parent.release();
}

// The in-call split of a large call (decode_device_split), when its conditions hold; nullptr: the call runs unsplit
static rh_device_result* try_split(rh_schema* s, const uint8_t* d_data, const uint64_t* d_offsets, uint64_t data_len, uint64_t n,
                                   uint64_t num_chunks, const rh_opts& o, rh_stats* stats, const ChunkGeo* geo) {
  const long G = env_long("RUHVRO_HIP_INTERNAL_STREAMS", kInternalStreamsDefault, 1, 8);
  const long groups_env = env_long("RUHVRO_HIP_SPLIT_GROUPS", 0, 0, 64);      // (> 1 with one stream: the groups run back to back)
  if (!(G > 1 || groups_env > 1) || geo || stats || n < (uint64_t)env_long("RUHVRO_HIP_SPLIT_MIN", kSplitMinDefault, 1, 1l << 40) ||
      (o.flags & 3) == RH_KERNEL_GENERIC || !(s->arena_ratio.load() > 0) || env_long("RUHVRO_HIP_TWO_SYNC", 0, 0, 1) != 0 ||
      env_long("RUHVRO_HIP_ARENA_PERMILLE", -1, 0, 1000000) >= 0)
    return nullptr;
  uint64_t k64 = rh_clamp_chunks(n, num_chunks), sz = n / std::max<uint64_t>(k64, 1);
  if (o.chunk_rows) {        // explicit geometry: refused by the unsplit path when it does not hold
    if (!explicit_geometry_ok(n, num_chunks, o.chunk_rows)) return nullptr;
    k64 = num_chunks; sz = o.chunk_rows;
  }
  const unsigned g = (unsigned)std::min<uint64_t>((uint64_t)G, k64);
  if (!(g > 1 || (groups_env > 1 && k64 > 1)) || ((uintptr_t)d_data & 15)) return nullptr;
  return decode_device_split(s, d_data, d_offsets, data_len, n, o, (uint32_t)k64, sz, n - (k64 - 1) * sz, g);
}

// ---------------------------------------------------------------------------
// The fall-back ladder.  A call that cannot finish on its form says so with an engine signal, and is repeated, synchronously,
// one rung down:
//   FORM_FIRST     as the caller asked: the single pass if it qualifies, a split over internal streams if that applies
//   FORM_TWO_PASS  NeedTwoPass (a single-pass call outgrew a capacity): the two-pass form, RH_INTERNAL_TWO_PASS
//   FORM_GENERIC   NeedWideIndex (a child row domain beyond 32-bit indexing; wide_fallbacks) or NeedRanged (a tile past the LDS
//                  window met specialised kernels without their ranged pair, which compiles in the background meanwhile;
//                  ranged_retries): the generic kernels.  Terminal: they raise none of the three.
// A signal that asks for a rung the call is already on (or past) propagates -- to guarded()'s last handler.  Every repeat comes
// back settled: a rung below the first clears RH_ASYNC.  The generic rung has ONE flag rule, (flags & ~(3 | RH_ASYNC)) |
// RH_KERNEL_GENERIC: the engine-internal bits stay, so the repeat of a host call keeps RH_INTERNAL_HOST_ARENA (as a host call in
// GENERIC mode has it from the start).
// ---------------------------------------------------------------------------
enum Form { FORM_FIRST, FORM_TWO_PASS, FORM_GENERIC };

// Called inside a catch (...): the rung the signal in flight asks for, counted.  Anything that is no signal, and a signal `now`
// cannot follow, is thrown on.
static Form next_rung(Form now) {
  try { throw; }
  catch (const NeedTwoPass&) { if (now != FORM_FIRST) throw; return FORM_TWO_PASS; }
  catch (const NeedWideIndex&) { if (now == FORM_GENERIC) throw; count(RH_CTR_WIDE_FALLBACKS); }
  catch (const NeedRanged&) { if (now == FORM_GENERIC) throw; count(RH_CTR_RANGED_RETRIES); }
  return FORM_GENERIC;
}

// The call on `form`, and on the rungs below it as long as it asks for them: at most three runs
static rh_device_result* decode_ladder(rh_schema* s, const uint8_t* d_data, const uint64_t* d_offsets, uint64_t data_len, uint64_t n,
                                       uint64_t num_chunks, rh_opts o, rh_stats* stats, const ChunkGeo* geo, Form form) {
  for (;;) {
    if (form == FORM_TWO_PASS) o.flags = (o.flags & ~RH_ASYNC) | RH_INTERNAL_TWO_PASS;
    if (form == FORM_GENERIC) o.flags = (o.flags & ~(3 | RH_ASYNC)) | RH_KERNEL_GENERIC;
    try {
      if (form == FORM_FIRST)
        if (rh_device_result* r = try_split(s, d_data, d_offsets, data_len, n, num_chunks, o, stats, geo)) return r;
      return decode_device_impl1(s, d_data, d_offsets, data_len, n, num_chunks, &o, stats, geo);
    } catch (...) {
      form = next_rung(form);
    }
  }
}

// The host's half of an asynchronous call (RH_ASYNC): wait for the stream, check for a malformed record, retry with an
// exact arena if the reserved one was too small, and take the call down the ladder if it asks for another form.  Throws what
// the synchronous call would have thrown; a failed result stays failed.
void settle(rh_device_result* r) {
  if (r->fail) std::rethrow_exception(r->fail);
  if (!r->parts.empty()) {
    // groups are settled in chunk order: the first failure is the lowest failing group's, i.e. the lowest malformed
    // record of the call (the in-order join of deserialize.rs:115-119)
    try {
      for (auto& p : r->parts) settle(p.get());
    } catch (...) {
      r->fail = std::current_exception();
      throw;
    }
    return;
  }
  if (!r->pending) return;
  std::unique_ptr<DeviceDecode> call = std::move(r->pending);
  try {
    Form next;
    try {
      call->finish();
      if (call->want_stats) { r->st = call->st; r->has_stats = true; }
      return;
    } catch (...) {
      next = next_rung(FORM_FIRST);
    }
    // the call again, synchronously, from the rung it asked for
    if (call->lean) lean_count(LC_RERUNS);
    call->drain();
    rh_stats st2;
    std::memset(&st2, 0, sizeof st2);
    std::unique_ptr<rh_device_result> r2(decode_ladder(call->s, call->d_data, call->d_offsets, call->data_len, call->n, call->num_chunks,
                                                       call->opts, call->want_stats ? &st2 : nullptr, call->geo, next));
    call.reset();                                  // (its reference to *r ends here)
    r->arena = std::move(r2->arena);
    r->arena_host = r2->arena_host;
    r->arena_bytes = r2->arena_bytes;
    r->buf_off = std::move(r2->buf_off); r->buf_size = std::move(r2->buf_size); r->dom_rows = std::move(r2->dom_rows);
    r->data_bytes = std::move(r2->data_bytes); r->nullcount = std::move(r2->nullcount); r->layout_bytes = std::move(r2->layout_bytes);
    r->output_bytes = r2->output_bytes; r->tables_done = r2->tables_done;
    r->k = r2->k; r->sz = r2->sz; r->rows_last = r2->rows_last;
    if (r2->has_stats || st2.records) { r->st = st2; r->has_stats = true; }
  } catch (...) {
    if (call) call->drain();
    r->arena.release();
    r->fail = std::current_exception();
    throw;
  }
}

rh_device_result* decode_device_impl(rh_schema* s, const uint8_t* d_data, const uint64_t* d_offsets, uint64_t data_len,
                                     uint64_t n, uint64_t num_chunks, const rh_opts* opts, rh_stats* stats,
                                     const ChunkGeo* geo) {
  return decode_ladder(s, d_data, d_offsets, data_len, n, num_chunks, opts ? *opts : default_opts(), stats, geo, FORM_FIRST);
}

}  // namespace rhe
