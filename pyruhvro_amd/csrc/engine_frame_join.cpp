// Framed messages, the write side: rh_frame_join puts the datums of several device-resident encode results
// (rh_encode_to_device, rh_encode_device) into message order and stamps a Confluent or single-object header in front of each, on
// the device.  The result is an rh_device_encoded like the ones it read: its accessors give the device-resident and the host form.
#include "engine_internal.h"
#include "frame_join.h"

extern "C" {
int rh_launch_join_lengths(const rh::JoinParams* J, void* stream);
int rh_launch_join_scan(const rh::JoinParams* J, void* stream);
int rh_launch_join_gather(const rh::JoinParams* J, void* stream);
}

using namespace rhe;

namespace rhe {

static std::mutex g_join_mu;
static float g_join_lengths_ms = 0, g_join_scan_ms = 0, g_join_gather_ms = 0;
static uint64_t g_join_n = 0;
static void note_join(float lengths_ms, float scan_ms, float gather_ms, uint64_t n) {
  std::lock_guard<std::mutex> g(g_join_mu);
  g_join_lengths_ms = lengths_ms; g_join_scan_ms = scan_ms; g_join_gather_ms = gather_ms; g_join_n = n;
}

// the layout of an encode result's arena (engine_encode.cpp): per chunk i32 offsets[rows + 1] | data
static std::unique_ptr<rh_device_encoded> lay_out(uint64_t n, uint64_t sz, uint64_t rows_last, uint32_t k, const std::vector<uint64_t>& totals,
                                                  int device) {
  auto res = std::make_unique<rh_device_encoded>();
  res->device = device; res->n = n; res->sz = sz; res->rows_last = rows_last; res->k = k;
  res->ooff.resize((size_t)k * 2);
  uint64_t otot = 0, exact = 0;
  for (uint32_t c = 0; c < k; c++) {
    const uint64_t rows = res->rows(c);
    res->ooff[(size_t)c * 2] = otot;
    otot += align_up((rows + 1) * 4, kAlign);
    res->ooff[(size_t)c * 2 + 1] = otot;
    otot += align_up(std::max<uint64_t>(totals[c], 8), kAlign);
    exact += (rows + 1) * 4 + totals[c];
  }
  res->out = Lease(dev_pool(), std::max<uint64_t>(otot, kAlign), device);
  res->out_bytes = std::max<uint64_t>(otot, 4);
  res->data_bytes = totals;
  res->exact = exact;
  return res;
}

static rh_device_encoded* frame_join(const rh_frame_source* src, uint32_t nsrc, uint32_t framing, uint64_t n, uint64_t num_chunks,
                                     const rh_opts* opts) {
  if (framing >= rh::FRAME_KINDS) throw std::invalid_argument("framed: unknown framing (0 = confluent, 1 = single_object)");
  if (nsrc && !src) throw std::invalid_argument("framed: null source list");
  if (opts && opts->n_devices > 0) throw std::invalid_argument("framed: a framed call runs on one device (rh_opts.devices is refused)");
  if (opts && (opts->flags & RH_ASYNC)) throw std::invalid_argument("framed: a framed call is synchronous: RH_ASYNC is refused");
  // ---- the sources: all on one device, their rows n together, indices on all of them or on none
  int device = -1;
  uint64_t rows = 0;
  uint32_t with_indices = 0, with_rows = 0;
  for (uint32_t s = 0; s < nsrc; s++) {
    const rh_device_encoded* e = src[s].enc;
    if (!e) throw std::invalid_argument("framed: source " + std::to_string(s) + " has no encode result");
    if (src[s].chunk >= e->k) throw std::invalid_argument("framed: source " + std::to_string(s) + " names chunk " + std::to_string(src[s].chunk) + " of " + std::to_string(e->k));
    if (framing == rh::FRAME_CONFLUENT && src[s].id > 0xFFFFFFFFull) throw std::invalid_argument("framed: a confluent schema id lies in 0 .. 2**32-1");
    if (device >= 0 && e->device != device) throw std::invalid_argument("framed: the sources live on more than one device");
    device = e->device;
    const uint64_t r = e->rows(src[s].chunk);
    rows += r;
    if (r) { with_rows++; with_indices += src[s].indices ? 1 : 0; }
  }
  if (rows != n) throw std::invalid_argument("framed: the sources have " + std::to_string(rows) + " rows, the call says " + std::to_string(n));
  if (with_indices && with_indices != with_rows) throw std::invalid_argument("framed: indices are given for some groups and not for others");
  require_device();
  if (opts && opts->device >= 0 && device >= 0 && opts->device != device) throw std::invalid_argument("framed: the sources live on another device");
  if (device < 0) {
    if (opts && opts->device >= 0) device = opts->device;
    else HIPCHK(hipGetDevice(&device));
  }
  HIPCHK(hipSetDevice(device));
  hipStream_t stream = opts ? (hipStream_t)opts->stream : nullptr;

  const uint32_t k = rh_clamp_chunks(n, num_chunks);
  const uint64_t sz = n / k, rows_last = n - (uint64_t)(k - 1) * sz;
  if (n == 0) {      // no launch: what an empty batch encodes to
    auto res = lay_out(0, sz, rows_last, k, std::vector<uint64_t>((size_t)k, 0), device);
    HIPCHK(hipMemsetAsync(res->out.ptr(), 0, 4, stream));
    HIPCHK(hipStreamSynchronize(stream));
    note_join(0, 0, 0, 0);
    return res.release();
  }
  const rh::FrameDesc d = rh::frame_desc(framing);

  // ---- the source table, in device memory (its size is not bounded by kernel-argument space); sources of no rows are left out
  std::vector<rh::JoinSource> table;
  std::vector<uint32_t> given;           // table entry -> position in src
  table.reserve(with_rows);
  uint64_t end = 0;
  for (uint32_t s = 0; s < nsrc; s++) {
    const rh_device_encoded* e = src[s].enc;
    const uint64_t r = e->rows(src[s].chunk);
    if (!r) continue;
    end += r;
    rh::JoinSource t;
    t.off = (const int32_t*)(e->out.ptr() + e->ooff[(size_t)src[s].chunk * 2]);
    t.data = e->out.ptr() + e->ooff[(size_t)src[s].chunk * 2 + 1];
    t.row_end = end;
    t.id = src[s].id;
    t.data_bytes = e->data_bytes[src[s].chunk];
    table.push_back(t);
    given.push_back(s);
  }
  const uint32_t m = (uint32_t)table.size();

  rh::JoinParams J;
  std::memset(&J, 0, sizeof J);
  J.nsrc = m; J.turns = rh::join_search_turns(m); J.kind = framing; J.k = k;
  J.n = n; J.ntiles = rh::join_tiles(n); J.sz = sz;
  if (J.ntiles > 0x7FFFFFFFull) throw std::invalid_argument("framed: too many messages for one call");

  // ---- workspace: ctrl [verdicts | k + 1 chunk bases] | source table | tile sums | tile prefixes | claim | len | who | at | abs
  const uint64_t ctrl_bytes = align_up(8ull * (rh::kJoinCtrlWords + k + 1), kAlign);
  const uint64_t o_table = ctrl_bytes;
  const uint64_t o_tsum = o_table + align_up(sizeof(rh::JoinSource) * (uint64_t)m, kAlign);
  const uint64_t o_tpre = o_tsum + align_up(8 * J.ntiles, kAlign);
  const uint64_t o_claim = o_tpre + align_up(8 * J.ntiles, kAlign);
  const uint64_t claim_bytes = with_indices ? align_up(4 * rh::join_claim_words(n), kAlign) : 0;
  const uint64_t o_len = o_claim + claim_bytes;
  const uint64_t o_who = o_len + align_up(4 * n, kAlign);
  const uint64_t o_at = o_who + align_up(4 * n, kAlign);
  const uint64_t o_abs = o_at + align_up(8 * n, kAlign);
  const uint64_t ws_bytes = o_abs + align_up(8 * (n + 1), kAlign);
  Lease ws(dev_pool(), ws_bytes, device);
  Lease didx;
  J.src = (const rh::JoinSource*)(ws.ptr() + o_table);
  J.ctrl = (unsigned long long*)ws.ptr();
  J.tile_sum = (uint64_t*)(ws.ptr() + o_tsum);
  J.tile_pre = (uint64_t*)(ws.ptr() + o_tpre);
  J.len = (uint32_t*)(ws.ptr() + o_len);
  J.who = (uint32_t*)(ws.ptr() + o_who);
  J.at = (uint64_t*)(ws.ptr() + o_at);
  J.abs = (uint64_t*)(ws.ptr() + o_abs);
  HIPCHK(hipMemsetAsync(ws.ptr(), 0xFF, 8ull * rh::kJoinCtrlWords, stream));      // kJoinNone
  HIPCHK(hipMemcpyAsync(ws.ptr() + o_table, table.data(), sizeof(rh::JoinSource) * (uint64_t)m, hipMemcpyHostToDevice, stream));
  if (with_indices) {
    J.claim = (uint32_t*)(ws.ptr() + o_claim);
    HIPCHK(hipMemsetAsync(J.claim, 0, claim_bytes, stream));
    didx = Lease(dev_pool(), 8 * n, device);
    J.indices = (const int64_t*)didx.ptr();
    for (uint32_t t = 0; t < m; t++) {
      const uint64_t first = t ? table[t - 1].row_end : 0;
      HIPCHK(hipMemcpyAsync(didx.ptr() + 8 * first, src[given[t]].indices, 8 * (table[t].row_end - first), hipMemcpyHostToDevice, stream));
    }
  }

  Events ev;
  ev.init();
  ev.rec(0, stream);
  if (rh_launch_join_lengths(&J, stream)) throw HipError("frame join (lengths) launch failed");
  ev.rec(1, stream);
  if (rh_launch_join_scan(&J, stream)) throw HipError("frame join (scan) launch failed");
  ev.rec(2, stream);
  std::vector<unsigned long long> ctrl((size_t)rh::kJoinCtrlWords + k + 1);
  HIPCHK(hipMemcpyAsync(ctrl.data(), J.ctrl, 8 * ctrl.size(), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));

  // ---- the verdicts: a damaged source, then the first index out of range, then the lowest position not named exactly once
  auto source_of_row = [&](uint64_t r, uint64_t* j) {
    const uint32_t t = rh::join_source_of(table.data(), m, r, J.turns);
    *j = rh::join_row_in_source(table.data(), t, r);
    return given[t];
  };
  if (ctrl[rh::kJoinBadSource] != rh::kJoinNone) {
    uint64_t j = 0;
    const uint32_t s = source_of_row(ctrl[rh::kJoinBadSource], &j);
    throw std::invalid_argument("framed: source " + std::to_string(s) + ": the offsets of row " + std::to_string(j) + " run backwards or past its data");
  }
  if (ctrl[rh::kJoinBadRange] != rh::kJoinNone) {
    uint64_t j = 0;
    const uint32_t s = source_of_row(ctrl[rh::kJoinBadRange], &j);
    throw DecodeError("framed: schema id " + std::to_string(src[s].id) + ": index " + std::to_string((long long)src[s].indices[j]) + " is outside 0 .. " +
                      std::to_string(n - 1));
  }
  if (with_indices) {
    // (every index is in range and there are n of them: a hole exists exactly when a position was named twice)
    uint64_t never = rh::kJoinNone, at = 0;
    if (ctrl[rh::kJoinBadTwice] != rh::kJoinNone) {
      std::vector<uint32_t> claim((size_t)rh::join_claim_words(n));
      HIPCHK(hipMemcpy(claim.data(), J.claim, 4 * claim.size(), hipMemcpyDeviceToHost));
      never = rh::join_lowest_hole(claim.data(), n);
    }
    const rh::JoinVerdict v = rh::join_perm_verdict(ctrl[rh::kJoinBadTwice], never, &at);
    if (v == rh::JOIN_TWICE) throw DecodeError("framed: position " + std::to_string(at) + " is named more than once");
    if (v == rh::JOIN_NEVER) throw DecodeError("framed: position " + std::to_string(at) + " is never named");
  }
  std::vector<uint64_t> totals((size_t)k);
  for (uint32_t c = 0; c < k; c++) {
    const uint64_t lo = ctrl[rh::kJoinCtrlWords + c], hi = ctrl[rh::kJoinCtrlWords + c + 1];
    if (hi < lo) throw std::runtime_error("internal error: the chunk bases of a frame join run backwards");
    totals[c] = hi - lo;
    if (totals[c] > 0x7FFFFFFFull)
      throw ValueClassError("framed: chunk " + std::to_string(c) + " holds " + std::to_string(totals[c]) +
                            " bytes of messages, past the 2**31-1 limit of BinaryArray offsets (raise num_chunks)");
  }
  (void)d;

  // ---- the result, leased like an encode's, and the gather
  auto res = lay_out(n, sz, rows_last, k, totals, device);
  std::vector<void*> outptr((size_t)k * 2);
  for (uint32_t c = 0; c < k; c++) {
    outptr[(size_t)c * 2] = res->out.ptr() + res->ooff[(size_t)c * 2];
    outptr[(size_t)c * 2 + 1] = res->out.ptr() + res->ooff[(size_t)c * 2 + 1];
  }
  Lease dptr(dev_pool(), align_up(16ull * k, kAlign), device);
  HIPCHK(hipMemcpyAsync(dptr.ptr(), outptr.data(), 16ull * k, hipMemcpyHostToDevice, stream));
  J.outptr = (void* const*)dptr.ptr();
  ev.rec(3, stream);
  if (rh_launch_join_gather(&J, stream)) throw HipError("frame join (gather) launch failed");
  ev.rec(4, stream);
  HIPCHK(hipStreamSynchronize(stream));
  note_join(ev.ms(0, 1), ev.ms(1, 2), ev.ms(3, 4), n);
  return res.release();
}

}  // namespace rhe

extern "C" {

int rh_frame_join(const rh_frame_source* src, uint32_t nsrc, uint32_t framing, uint64_t n, uint64_t num_chunks, const rh_opts* opts,
                  rh_device_encoded** out, char** err) {
  if (!out) return RH_ERR_ARGUMENT;
  *out = nullptr;
  return guarded(err, [&] {
    *out = frame_join(src, nsrc, framing, n, num_chunks, opts);
    return (int)RH_OK;
  });
}

void rh_frame_join_last(float* lengths_ms, float* scan_ms, float* gather_ms, uint64_t* n) {
  std::lock_guard<std::mutex> g(g_join_mu);
  if (lengths_ms) *lengths_ms = g_join_lengths_ms;
  if (scan_ms) *scan_ms = g_join_scan_ms;
  if (gather_ms) *gather_ms = g_join_gather_ms;
  if (n) *n = g_join_n;
}

}  // extern "C"
