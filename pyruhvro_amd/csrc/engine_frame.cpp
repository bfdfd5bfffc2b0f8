// Framed messages: Kafka-framed Avro -- Confluent wire format or Avro single-object encoding -- checked, split by
// writer schema id and stripped of its headers on the device (rh_frame_split_packed / rh_frame_split_device), and the unchanged
// strict decode of one class's payloads with that class's schema (rh_frame_decode_class).  Every class gets leases of its own for
// its payload and its offsets, which its decode's result takes over as a filtered call's result takes over the compacted list.
#include "engine_internal.h"
#include "frame.h"

extern "C" {
int rh_launch_frame_classify(const rh::FrameParams* F, void* stream);
int rh_launch_frame_scan(const rh::FrameParams* F, void* stream);
int rh_launch_frame_offsets(const rh::FrameParams* F, void* stream);
int rh_launch_frame_gather(const rh::FrameParams* F, void* stream);
}

using namespace rhe;

struct rh_frame_split {
  int device = 0;
  uint32_t kind = 0, m = 0, flags = 0;
  uint64_t n = 0;
  uint64_t ids[rh::kMaxFrameIds];
  uint64_t count[rh::kFrameBins];            // messages of every bin (bin m: unknown ids)
  uint64_t bytes[rh::kFrameBins];            // payload bytes of every class
  uint64_t index_base[rh::kFrameBins];
  Lease cls;                                 // [n] verdict bytes
  Lease indices;                             // [n] int64, bin by bin
  Lease payload[rh::kMaxFrameIds];           // class c: bytes[c] payload bytes + kFrameSlack zero bytes
  Lease offsets[rh::kMaxFrameIds];           // class c: count[c] + 1 offsets
  bool taken[rh::kMaxFrameIds];              // ... handed to a decode's result
};

namespace rhe {

static const char* const kFramingName[rh::FRAME_KINDS] = {"confluent", "single_object"};

static std::mutex g_frame_mu;
static float g_classify_ms = 0, g_scan_offsets_ms = 0, g_gather_ms = 0;
static uint64_t g_frame_n = 0;
static void note_frame(float classify_ms, float scan_offsets_ms, float gather_ms, uint64_t n) {
  std::lock_guard<std::mutex> g(g_frame_mu);
  g_classify_ms = classify_ms; g_scan_offsets_ms = scan_offsets_ms; g_gather_ms = gather_ms; g_frame_n = n;
}

static void refuse_frame_opts(const rh_opts* opts) {
  if (opts && opts->n_devices > 0) throw std::invalid_argument("framed: a framed call runs on one device (rh_opts.devices is refused)");
  if (opts && (opts->flags & RH_ASYNC)) throw std::invalid_argument("framed: a framed call is synchronous: RH_ASYNC is refused");
}

static void check_ids(const uint64_t* ids, uint32_t m, uint32_t framing) {
  if (framing >= rh::FRAME_KINDS) throw std::invalid_argument("framed: unknown framing (0 = confluent, 1 = single_object)");
  if (m < 1 || m > rh::kMaxFrameIds) throw std::invalid_argument("framed: 1 to 32 schemas per call");
  if (!ids) throw std::invalid_argument("framed: null id list");
  for (uint32_t c = 0; c < m; c++) {
    if (c && ids[c] <= ids[c - 1]) throw std::invalid_argument("framed: the schema ids must be ascending and distinct");
    if (framing == rh::FRAME_CONFLUENT && ids[c] > 0xFFFFFFFFull) throw std::invalid_argument("framed: a confluent schema id lies in 0 .. 2**32-1");
  }
}

// the message of the lowest failing index, from what the device holds of it
[[noreturn]] static void framing_fail(const rh::FrameParams& F, uint64_t i, hipStream_t stream) {
  const rh::FrameDesc d = rh::frame_desc(F.kind);
  uint64_t be[2] = {0, 0};
  uint8_t v = 0;
  HIPCHK(hipMemcpyAsync(be, F.offsets + i, 16, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(&v, F.cls + i, 1, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  const std::string at = "framed: message " + std::to_string(i);
  const char* const name = kFramingName[F.kind];
  if (v == rh::kFrameShort) {
    const uint64_t len = be[1] >= be[0] ? be[1] - be[0] : 0;
    throw DecodeError(at + " is " + std::to_string(len) + " bytes, shorter than the " + std::to_string(d.header) + "-byte " + name + " header");
  }
  if (v == rh::kFrameBadMarker) throw DecodeError(at + " does not start with the " + name + " marker");
  if (v != rh::kFrameUnknown) throw std::runtime_error("internal error: the framing failure of message " + std::to_string(i) + " has verdict " + std::to_string(v));
  uint8_t head[rh::kFrameMaxHeader] = {0};
  HIPCHK(hipMemcpy(head, F.data + be[0], d.header, hipMemcpyDeviceToHost));
  throw DecodeError(at + " carries schema id " + std::to_string(rh::frame_id(head, d)) + ", which is not in schemas");
}

static std::unique_ptr<rh_frame_split> split_device(const uint8_t* d_data, const uint64_t* d_offsets, uint64_t data_len, uint64_t n,
                                                    const uint64_t* ids, uint32_t m, uint32_t framing, uint32_t flags, int device,
                                                    hipStream_t stream) {
  std::unique_ptr<rh_frame_split> sp(new rh_frame_split);
  sp->device = device; sp->kind = framing; sp->m = m; sp->flags = flags; sp->n = n;
  for (uint32_t c = 0; c < rh::kFrameBins; c++) { sp->count[c] = sp->bytes[c] = sp->index_base[c] = 0; }
  for (uint32_t c = 0; c < rh::kMaxFrameIds; c++) { sp->ids[c] = c < m ? ids[c] : 0; sp->taken[c] = false; }
  const bool classify_only = (flags & RH_FRAME_CLASSIFY_ONLY) != 0;
  if (n == 0) {      // no launch: every class is the empty list
    if (!classify_only)
      for (uint32_t c = 0; c < m; c++) {
        sp->payload[c] = Lease(dev_pool(), rh::kFrameSlack, device);
        sp->offsets[c] = Lease(dev_pool(), 8, device);
        HIPCHK(hipMemsetAsync(sp->payload[c].ptr(), 0, rh::kFrameSlack, stream));
        HIPCHK(hipMemsetAsync(sp->offsets[c].ptr(), 0, 8, stream));
      }
    HIPCHK(hipStreamSynchronize(stream));
    note_frame(0, 0, 0, 0);
    return sp;
  }
  if ((uintptr_t)d_data & 15) throw std::invalid_argument("device payload pointer must be 16-byte aligned");
  if (!d_data || !d_offsets) throw std::invalid_argument("framed: null device input");

  rh::FrameParams F;
  std::memset(&F, 0, sizeof F);
  F.data = d_data; F.offsets = d_offsets; F.data_len = data_len; F.n = n; F.ntiles = rh::frame_tiles(n);
  F.kind = framing; F.m = m; F.skip_unknown = (flags & (RH_FRAME_SKIP_UNKNOWN | RH_FRAME_CLASSIFY_ONLY)) ? 1 : 0;
  for (uint32_t c = 0; c < m; c++) F.ids[c] = ids[c];
  if (F.ntiles > 0x7FFFFFFFull) throw std::invalid_argument("framed: too many messages for one call");
  const uint64_t table = align_up(8ull * (m + 1) * F.ntiles, kAlign);
  const uint64_t o_totals = 4 * table;
  const uint64_t o_bad = o_totals + align_up(16ull * (m + 1), kAlign);
  Lease ws(dev_pool(), o_bad + kAlign, device);
  sp->cls = Lease(dev_pool(), n, device);
  F.cls = sp->cls.ptr();
  F.tile_cnt = (uint64_t*)ws.ptr(); F.tile_bytes = (uint64_t*)(ws.ptr() + table);
  F.pre_cnt = (uint64_t*)(ws.ptr() + 2 * table); F.pre_bytes = (uint64_t*)(ws.ptr() + 3 * table);
  F.totals = (uint64_t*)(ws.ptr() + o_totals);
  F.first_bad = (unsigned long long*)(ws.ptr() + o_bad);

  Events ev;
  ev.init();
  struct { uint64_t totals[2 * rh::kFrameBins]; } head;
  unsigned long long first_bad = 0;
  HIPCHK(hipMemsetAsync(F.first_bad, 0xFF, 8, stream));      // kFrameNoFailure
  ev.rec(0, stream);
  if (rh_launch_frame_classify(&F, stream)) throw HipError("frame (classify) launch failed");
  ev.rec(1, stream);
  HIPCHK(hipMemcpyAsync(&first_bad, F.first_bad, 8, hipMemcpyDeviceToHost, stream));
  if (!classify_only) {
    if (rh_launch_frame_scan(&F, stream)) throw HipError("frame (scan) launch failed");
    ev.rec(2, stream);
    HIPCHK(hipMemcpyAsync(head.totals, F.totals, 16ull * (m + 1), hipMemcpyDeviceToHost, stream));
  }
  HIPCHK(hipStreamSynchronize(stream));
  if (first_bad != rh::kFrameNoFailure) {
    if (first_bad >= n) throw std::runtime_error("internal error: a framing failure past the last message");
    framing_fail(F, first_bad, stream);
  }
  if (classify_only) {
    note_frame(ev.ms(0, 1), 0, 0, n);
    return sp;
  }
  uint64_t seen = 0;
  for (uint32_t c = 0; c <= m; c++) {
    sp->count[c] = head.totals[c];
    sp->bytes[c] = head.totals[(m + 1) + c];
    sp->index_base[c] = seen;
    seen += sp->count[c];
    if (sp->bytes[c] > data_len) throw std::runtime_error("internal error: a class's payloads are larger than the input");
  }
  if (seen != n) throw std::runtime_error("internal error: the classes do not partition the messages");
  sp->indices = Lease(dev_pool(), 8 * n, device);
  Lease dst(dev_pool(), 8 * n, device);
  F.indices = (int64_t*)sp->indices.ptr();
  F.dst = (uint64_t*)dst.ptr();
  for (uint32_t c = 0; c <= m; c++) F.index_base[c] = sp->index_base[c];
  for (uint32_t c = 0; c < m; c++) {
    sp->payload[c] = Lease(dev_pool(), sp->bytes[c] + rh::kFrameSlack, device);
    sp->offsets[c] = Lease(dev_pool(), 8 * (sp->count[c] + 1), device);
    F.out[c] = sp->payload[c].ptr();
    F.new_offsets[c] = (uint64_t*)sp->offsets[c].ptr();
  }
  ev.rec(3, stream);
  if (rh_launch_frame_offsets(&F, stream)) throw HipError("frame (offsets) launch failed");
  ev.rec(4, stream);
  if (rh_launch_frame_gather(&F, stream)) throw HipError("frame (gather) launch failed");
  ev.rec(5, stream);
  for (uint32_t c = 0; c < m; c++) HIPCHK(hipMemsetAsync(sp->payload[c].ptr() + sp->bytes[c], 0, rh::kFrameSlack, stream));
  HIPCHK(hipStreamSynchronize(stream));      // (a decode that deals its chunk groups to internal streams reads the regions from those)
  note_frame(ev.ms(0, 1), ev.ms(1, 2) + ev.ms(3, 4), ev.ms(4, 5), n);
  return sp;
}

static int frame_device(const rh_opts* opts) {
  int device = 0;
  if (opts && opts->device >= 0) { HIPCHK(hipSetDevice(opts->device)); return opts->device; }
  HIPCHK(hipGetDevice(&device));
  return device;
}

static const rh_frame_split* settled(const rh_frame_split* sp, uint32_t bin) {
  if (!sp) throw std::invalid_argument("framed: null split");
  if (sp->flags & RH_FRAME_CLASSIFY_ONLY) throw std::invalid_argument("framed: the split was made with RH_FRAME_CLASSIFY_ONLY: it has verdicts only");
  if (bin > sp->m) throw std::invalid_argument("framed: no such class");
  return sp;
}

}  // namespace rhe

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

int rh_frame_split_device(const void* d_data, const void* d_offsets, uint64_t data_len, uint64_t n, const uint64_t* ids, uint32_t m,
                          uint32_t framing, uint32_t flags, const rh_opts* opts, rh_frame_split** out, char** err) {
  if (!out) return RH_ERR_ARGUMENT;
  *out = nullptr;
  return guarded(err, [&] {
    check_ids(ids, m, framing);
    refuse_frame_opts(opts);
    require_device();
    const int device = frame_device(opts);
    *out = split_device((const uint8_t*)d_data, (const uint64_t*)d_offsets, data_len, n, ids, m, framing, flags, device,
                        opts ? (hipStream_t)opts->stream : nullptr).release();
    return RH_OK;
  });
}

int rh_frame_split_packed(const uint8_t* data, const uint64_t* offsets, uint64_t n, const uint64_t* ids, uint32_t m, uint32_t framing,
                          uint32_t flags, const rh_opts* opts, rh_frame_split** out, char** err) {
  if (!out || !offsets) return RH_ERR_ARGUMENT;
  *out = nullptr;
  return guarded(err, [&] {
    check_ids(ids, m, framing);
    refuse_frame_opts(opts);
    require_device();
    const int device = frame_device(opts);
    hipStream_t stream = opts ? (hipStream_t)opts->stream : nullptr;
    Source src;
    src.data = data;
    src.offsets = offsets;
    Uploaded u;
    upload(src, n, device, stream, u);      // (the split keeps nothing of it: the payloads are copied into the classes' regions)
    *out = split_device(u.data.ptr(), (const uint64_t*)u.off.ptr(), u.bytes, n, ids, m, framing, flags, device, stream).release();
    return RH_OK;
  });
}

uint64_t rh_frame_split_count(const rh_frame_split* sp, uint32_t c) { return (sp && c <= sp->m) ? sp->count[c] : 0; }

int rh_frame_split_classes(const rh_frame_split* sp, uint8_t* out, char** err) {
  return guarded(err, [&] {
    if (!sp || (!out && sp->n)) throw std::invalid_argument("framed: null split or output");
    if (sp->n) {
      HIPCHK(hipSetDevice(sp->device));
      HIPCHK(hipMemcpy(out, sp->cls.ptr(), sp->n, hipMemcpyDeviceToHost));
    }
    return RH_OK;
  });
}

int rh_frame_split_indices(const rh_frame_split* sp, uint32_t c, int64_t* out, char** err) {
  return guarded(err, [&] {
    settled(sp, c);
    if (sp->count[c]) {
      if (!out) throw std::invalid_argument("framed: null output");
      HIPCHK(hipSetDevice(sp->device));
      HIPCHK(hipMemcpy(out, sp->indices.ptr() + 8 * sp->index_base[c], 8 * sp->count[c], hipMemcpyDeviceToHost));
    }
    return RH_OK;
  });
}

int rh_frame_decode_class(rh_frame_split* sp, uint32_t c, const rh_schema* s, uint64_t num_chunks, const rh_opts* opts,
                          struct ArrowArray* out_chunks, uint32_t* out_k, rh_stats* stats, char** err) {
  if (!s || !out_chunks) return RH_ERR_ARGUMENT;
  return guarded(err, [&] {
    settled(sp, c);
    if (c >= sp->m) throw std::invalid_argument("framed: no such class");
    if (sp->taken[c]) throw std::invalid_argument("framed: the class was decoded already (its result owns the payloads)");
    refuse_frame_opts(opts);
    Timer t;
    rh_opts pub;
    if (opts) { pub = *opts; pub.flags &= kPublicFlags; }
    if (opts && opts->device >= 0 && opts->device != sp->device) throw std::invalid_argument("framed: the split lives on another device");
    HIPCHK(hipSetDevice(sp->device));
    hipStream_t stream = opts ? (hipStream_t)opts->stream : nullptr;
    std::unique_ptr<rh_device_result> r;
    try {
      r.reset(decode_device_impl(const_cast<rh_schema*>(s), sp->payload[c].ptr(), (const uint64_t*)sp->offsets[c].ptr(), sp->bytes[c],
                                 sp->count[c], num_chunks, opts ? &pub : nullptr, stats));
    } catch (const DecodeError& e) {
      throw DecodeError("framed: schema id " + std::to_string(sp->ids[c]) + ": " + e.what());
    }
    sp->taken[c] = true;
    r->patched_data = std::move(sp->payload[c]);      // the result owns every byte its call read (as a filtered call's)
    r->patched_offsets = std::move(sp->offsets[c]);
    Timer td;
    const int rc = to_host_impl(r.get(), out_chunks, stream);
    if (stats) stats->d2h_ms = td.ms();
    if (out_k) *out_k = r->k;
    if (stats) stats->total_ms = t.ms();
    return rc;
  });
}

void rh_frame_split_free(rh_frame_split* sp) { delete sp; }

void rh_frame_last(float* classify_ms, float* scan_offsets_ms, float* gather_ms, uint64_t* n) {
  std::lock_guard<std::mutex> g(g_frame_mu);
  if (classify_ms) *classify_ms = g_classify_ms;
  if (scan_offsets_ms) *scan_offsets_ms = g_scan_offsets_ms;
  if (gather_ms) *gather_ms = g_gather_ms;
  if (n) *n = g_frame_n;
}

}  // extern "C"
