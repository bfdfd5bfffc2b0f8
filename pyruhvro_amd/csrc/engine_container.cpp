// Avro object container files: the framing scan behind the C ABI (rh_container_scan: host only) and the
// blocks entry points (rh_decode_blocks / rh_decode_blocks_device): the file uploaded as it is, rh_k_split (container.hip)
// turning the block table into record offsets, then the device-input decode (decode_device_impl) on (d_data, d_offsets, n).
// Deflate blocks in both directions: rh_decode_cblocks / rh_inflate_blocks (inflate.hip) and rh_deflate_blocks
// with its host twin (deflate.hip, deflate_core.h).
#include "engine_internal.h"
#include "container.h"
#include "container_scan.h"
#include "inflate.h"
#include "deflate.h"

extern "C" {
uint32_t rh_split_lds_bytes(int list_depth);
int rh_launch_split(const rh::SParams* S, void* stream);
int rh_launch_split_where(const rh::SWParams* W, void* stream);
int rh_launch_split_salvage(const rh::SalvageParams* P, void* stream);
int rh_launch_salvage_gather(const rh::SalvageGatherParams* G, void* stream);
int rh_launch_inflate_size(const rh::InflateParams* P, void* stream);
int rh_launch_inflate_emit(const rh::InflateParams* P, void* stream);
int rh_launch_deflate(const rh::DeflateParams* P, void* stream);
int rh_launch_deflate_gather(const rh::DeflateGatherParams* P, void* stream);
}

using namespace rhe;

struct rh_container_info {
  rhc::ContainerInfo ci;
  rhc::SalvageInfo sv;      // rh_container_salvage: everything but sv.info, which is moved into ci
  bool salvaged = false;
};

namespace rhe {

static std::atomic<float> g_split_last_ms{0.0f};

// The predicate of a filtered container read (rh_decode_*blocks*_where, rh_filter_*blocks).
struct WhereCall {
  rh_filter* f = nullptr;
  bool mask_only = false;            // rh_filter_blocks / rh_filter_cblocks: the split and the predicate alone, no decode
  uint64_t* keep_words = nullptr;    // ... their out: host room for ceil(n / 64) words
  uint64_t kept = 0;                 // out
};
static std::mutex g_where_last_mu;
static struct { float split_ms = 0, gather_ms = 0; uint64_t n = 0, kept = 0; } g_where_last;
static void note_where(float split_ms, float gather_ms, uint64_t n, uint64_t kept) {
  std::lock_guard<std::mutex> g(g_where_last_mu);
  g_where_last.split_ms = split_ms; g_where_last.gather_ms = gather_ms; g_where_last.n = n; g_where_last.kept = kept;
}
static constexpr uint64_t kMaxEmptyRecords = 1ull << 24;

// The split walks the WRITER's plain program.  A projection or a resolution keeps the writer's text (CompiledSchema::json)
// but its program carries F_DROP / resolution ops: the plain compile of that text, made on first use and owned by `s`.
static rh_schema* plain_schema(rh_schema* s) {
  if (!s->cs->projected) return s;
  std::lock_guard<std::mutex> g(s->mu);
  if (!s->plain_parent) {
    std::unique_ptr<rh_schema> p(new rh_schema());
    p->cs = rh::compile_schema(s->cs->json.data(), s->cs->json.size());
    s->plain_parent = p.release();
  }
  return s->plain_parent;
}

// What every blocks call refuses before it looks at a block.
static void check_blocks_call(const rh_opts* opts, const uint8_t* data, const uint64_t* start, const uint64_t* end, const uint64_t* first, uint64_t nb) {
  if (opts && opts->n_devices > 0) throw std::invalid_argument("container: a container is read on one device (rh_opts.devices is refused)");
  if (opts && (opts->flags & RH_ASYNC)) throw std::invalid_argument("container: the blocks call is synchronous: RH_ASYNC is refused");
  if (opts && opts->chunk_rows) throw std::invalid_argument("container: chunk_rows applies to rh_decode_device only");
  if (nb > 0xFFFFFFFFull) throw std::invalid_argument("container: more than 2^32 - 1 blocks");
  if (nb && (!start || !end || !data)) throw std::invalid_argument("container: null block table");
  if (!first || first[0] != 0) throw std::invalid_argument("container: first[0] must be 0");
}

static std::string block_where(uint64_t b) { return "container: block " + std::to_string(b) + ": "; }      // (error paths only)

// The messages of a block: built here for the strict calls, which throw them, and for the tolerant ones, which report them.
static std::string block_large_message(uint64_t b, uint64_t size) {
  return block_where(b) + "a block of 4 GiB - 16 bytes or more is not supported (" + std::to_string(size) + " bytes)";
}
static std::string block_count_message(uint64_t b, uint64_t cnt, uint64_t size) {
  return block_where(b) + std::to_string(cnt) + " records cannot be in its " + std::to_string(size) + " bytes";
}
static std::string block_end_message(uint64_t b, uint64_t cnt, int64_t at, uint64_t size) {
  return "container: block " + std::to_string(b) + ": its " + std::to_string(cnt) + " records end at byte " + std::to_string(at) + " of " + std::to_string(size);
}
// The checks of one block of UNCOMPRESSED bytes: its size, and what bounds a lane's loop, and through it the call's records and
// its offsets: every record has its minimum wire bytes.
static bool block_too_large(uint64_t size) { return size >= 0xFFFFFFF0ull; }
static bool block_count_refused(uint64_t size, uint64_t cnt, uint64_t min_rec) { return min_rec && cnt > size / min_rec; }

static void check_block_size(uint64_t b, uint64_t size, uint64_t cnt, uint64_t min_rec) {
  if (block_too_large(size)) throw DecodeError(block_large_message(b, size));
  if (block_count_refused(size, cnt, min_rec)) throw DecodeError(block_count_message(b, cnt, size));
}

// records of no bytes at all (a schema of empty records) are bounded by no byte count: by a count for the whole call, which
// bounds every block's loop too -- a small file of many such blocks may not size the offsets
static void check_empty_records(uint64_t min_rec, uint64_t n) {
  if (!min_rec && n > kMaxEmptyRecords)
    throw DecodeError("container: " + std::to_string(n) + " records of a schema whose records may be empty: at most " +
                      std::to_string(kMaxEmptyRecords) + " in one call");
}

// The table of a blocks call on the device: start[nb], end[nb], first[nb + 1], the split's verdicts.
struct BlockTable {
  Lease d_tab, d_off;
  uint64_t o_end = 0, o_first = 0, o_err = 0, o_bad = 0;
  void upload(const uint64_t* start, const uint64_t* end, const uint64_t* first, uint64_t nb, uint64_t n, int device, hipStream_t stream) {
    d_off = Lease(dev_pool(), 8 * (n + 1), device);
    o_end = 8 * nb; o_first = 16 * nb; o_err = align_up(o_first + 8 * (nb + 1), 16); o_bad = o_err + sizeof(rh::SplitErr) * nb;
    d_tab = Lease(dev_pool(), o_bad + 8, device);
    if (nb) {
      HIPCHK(hipMemcpyAsync(d_tab.ptr(), start, 8 * nb, hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(d_tab.ptr() + o_end, end, 8 * nb, hipMemcpyHostToDevice, stream));
    }
    HIPCHK(hipMemcpyAsync(d_tab.ptr() + o_first, first, 8 * (nb + 1), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemsetAsync(d_tab.ptr() + o_err, 0, o_bad + 8 - o_err, stream));
    if (nb == 0) HIPCHK(hipMemsetAsync(d_off.ptr(), 0, 8, stream));      // (no block, no lane: offsets[0] = 0)
  }
};

// Both roads from "the table and the bytes are on the device" onward: the split launch, its verdict, the device-input decode,
// and the result's ownership of the buffers.  d_data holds `len` bytes of uncompressed blocks at [start[b], end[b]) (+ slack).
// W: the call's predicate.  The split launch is then rh_k_split_where -- the same walk, the same offsets and
// verdicts, and a keep bit per record -- and what is decoded is what the predicate keeps: everything (the buffers as they are,
// no compaction launch), or the compacted list (compact_kept, as a filtered list call's).  W->mask_only: the call ends behind
// the split with the keep words on the host, and returns nullptr.
static rh_device_result* split_and_decode(rh_schema* s, rh_schema* plain, Lease& d_data, uint64_t len, BlockTable& T, const uint64_t* start,
                                          const uint64_t* end, const uint64_t* first, uint64_t nb, uint64_t num_chunks, const rh_opts* opts,
                                          rh_stats* stats, int device, hipStream_t stream, float up_ms, WhereCall* W = nullptr) {
  Lease& d_off = T.d_off;
  Lease& d_tab = T.d_tab;
  const uint64_t o_end = T.o_end, o_first = T.o_first, o_err = T.o_err, o_bad = T.o_bad;
  const uint64_t n = first[nb];
  const uint64_t data_end = nb ? end[nb - 1] : 0;
  float split_ms = 0;
  Lease d_keep;      // W: the keep words, the kept slots, the byte comparands
  if (nb) {
    // (W: the predicate's pcs point into the filter's own plain compile of the same writer text)
    rh_schema* const walked = W ? W->f->plain : plain;
    const DeviceProgram& dp = device_program(walked, device);
    rh::SWParams SW;
    std::memset(&SW, 0, sizeof SW);
    rh::SParams& S = SW.S;
    S.data = d_data.ptr(); S.data_len = len;
    S.start = (const uint64_t*)d_tab.ptr(); S.end = (const uint64_t*)(d_tab.ptr() + o_end); S.first = (const uint64_t*)(d_tab.ptr() + o_first);
    S.nb = (uint32_t)nb; S.list_depth = walked->cs->list_depth;
    S.prog = dp.prog; S.sym_off = dp.sym_off; S.sym_data = dp.sym_data;
    S.offsets = (uint64_t*)d_off.ptr();
    S.err = (rh::SplitErr*)(d_tab.ptr() + o_err);
    S.first_bad = (unsigned long long*)(d_tab.ptr() + o_bad);
    if (rh_split_lds_bytes(S.list_depth) > 160 * 1024 - 512) throw rh::SchemaError("schema needs more LDS than a CDNA4 workgroup has");
    unsigned long long slots[rh::kFilterSlots] = {};
    if (W) {
      const uint64_t o_kept = align_up(8 * rh::filter_words(n), kAlign);
      const uint64_t o_bytes = o_kept + align_up(8 * rh::kFilterSlots, kAlign);
      const uint64_t o_prog = o_bytes + align_up(std::max<uint64_t>(W->f->bytes.size(), 1), kAlign);
      d_keep = Lease(dev_pool(), o_prog + align_up(sizeof(rh::FilterProgram), kAlign), device);
      SW.keep = (uint64_t*)d_keep.ptr(); SW.kept = (unsigned long long*)(d_keep.ptr() + o_kept); SW.cbytes = d_keep.ptr() + o_bytes;
      SW.flt = (const rh::FilterProgram*)(d_keep.ptr() + o_prog);
      HIPCHK(hipMemsetAsync(d_keep.ptr(), 0, o_bytes, stream));      // (the lanes OR their bits into zeroed words)
      HIPCHK(hipMemcpyAsync(d_keep.ptr() + o_prog, &W->f->prog, sizeof(rh::FilterProgram), hipMemcpyHostToDevice, stream));
      if (!W->f->bytes.empty()) HIPCHK(hipMemcpyAsync(d_keep.ptr() + o_bytes, W->f->bytes.data(), W->f->bytes.size(), hipMemcpyHostToDevice, stream));
    }
    Events ev;
    ev.init();
    ev.rec(0, stream);
    if (W) {
      if (rh_launch_split_where(&SW, stream)) throw HipError("k_split_where launch failed");
    } else if (rh_launch_split(&S, stream)) throw HipError("k_split launch failed");
    ev.rec(1, stream);
    unsigned long long fb = 0;
    HIPCHK(hipMemcpyAsync(&fb, S.first_bad, 8, hipMemcpyDeviceToHost, stream));
    if (W) HIPCHK(hipMemcpyAsync(slots, SW.kept, sizeof slots, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    split_ms = ev.ms(0, 1);
    if (fb) {
      const unsigned long long key = ~fb;
      std::vector<rh::SplitErr> errs(nb);
      HIPCHK(hipMemcpy(errs.data(), S.err, sizeof(rh::SplitErr) * nb, hipMemcpyDeviceToHost));
      if (key & 1ull) {      // the lowest malformed record: what the list decode raises for it
        const uint64_t rec = (key - 1) / 2;
        const uint64_t b = (uint64_t)(std::upper_bound(first, first + nb + 1, rec) - first) - 1;
        rh::ErrInfo ei; ei.code = errs[b].code; ei.pad = 0; ei.detail = errs[b].detail;
        throw RecordDecodeError(format_error(ei));
      }
      const uint64_t fn = key / 2;
      for (uint64_t b = (uint64_t)(std::lower_bound(first + 1, first + nb + 1, fn) - (first + 1)); b < nb && first[b + 1] == fn; b++)
        if (errs[b].code == rh::E_BLOCK_END)
          throw DecodeError(block_end_message(b, first[b + 1] - first[b], errs[b].detail, end[b] - start[b]));
      throw std::runtime_error("internal error: the split kernel reported a failure no block owns");
    }
    if (W) {
      W->kept = 0;
      for (uint32_t i = 0; i < rh::kFilterSlots; i++) W->kept += slots[i];
      if (W->kept > n) throw std::runtime_error("internal error: the filter kept more records than it was given");
    }
  }
  g_split_last_ms.store(split_ms);

  if (W && W->mask_only) {
    if (n && W->keep_words) HIPCHK(hipMemcpy(W->keep_words, d_keep.ptr(), 8 * rh::filter_words(n), hipMemcpyDeviceToHost));
    note_where(split_ms, 0, n, W->kept);
    return nullptr;
  }
  if (W && W->kept != n) {
    Compacted c;
    compact_kept(d_data.ptr(), (const uint64_t*)d_off.ptr(), data_end, n, (const uint64_t*)d_keep.ptr(), W->kept, device, stream, c);
    note_where(split_ms, c.ms, n, W->kept);
    d_keep.release();
    d_data.release();      // (the kept records have buffers of their own: the file goes back to the pool before the decode)
    d_off.release();
    rh_device_result* r;
    try {
      r = decode_device_impl(s, c.data.ptr(), (const uint64_t*)c.off.ptr(), c.len, W->kept, num_chunks, opts, stats);
    } catch (const RecordDecodeError& e) {
      throw std::runtime_error(std::string("internal error: a record the split accepted failed to decode: ") + e.what());
    }
    r->patched_data = std::move(c.data);      // the result owns the compacted buffers, as a filtered list call's
    r->patched_offsets = std::move(c.off);
    if (stats) stats->h2d_ms += up_ms;
    return r;
  }
  if (W) {
    note_where(split_ms, 0, n, W->kept);
    d_keep.release();
  }

  rh_device_result* r = decode_device_impl(s, d_data.ptr(), (const uint64_t*)d_off.ptr(), data_end, n, num_chunks, opts, stats);
  r->container_data = std::move(d_data);      // the result owns every byte its call read (as a repaired tolerant call's)
  r->container_offsets = std::move(d_off);
  if (stats) stats->h2d_ms += up_ms;
  return r;
}

static rh_device_result* decode_blocks_impl(rh_schema* s, const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end,
                                            const uint64_t* first, uint64_t nb, uint64_t num_chunks, const rh_opts* opts, rh_stats* stats,
                                            WhereCall* W = nullptr) {
  check_blocks_call(opts, data, start, end, first, nb);
  if (W) check_filter(s, W->f);
  rh_schema* const plain = plain_schema(s);
  const uint64_t min_rec = plain->cs->min_record_bytes;
  for (uint64_t b = 0; b < nb; b++) {
    if (start[b] > end[b] || end[b] > len || (b && start[b] < end[b - 1])) throw std::invalid_argument(block_where(b) + "its bytes are outside the buffer or out of order");
    if (first[b + 1] < first[b]) throw std::invalid_argument(block_where(b) + "negative record count");
    check_block_size(b, end[b] - start[b], first[b + 1] - first[b], min_rec);
  }
  const uint64_t n = first[nb];
  check_empty_records(min_rec, n);

  require_device();
  int device = 0;
  if (opts && opts->device >= 0) { HIPCHK(hipSetDevice(opts->device)); device = opts->device; }
  else HIPCHK(hipGetDevice(&device));
  hipStream_t stream = opts ? (hipStream_t)opts->stream : nullptr;

  // the file as it is (+ slack behind it), the table, the offsets, the verdict
  Timer t_up;
  Lease d_data(dev_pool(), len + 64, device);
  if (len) HIPCHK(hipMemcpyAsync(d_data.ptr(), data, len, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemsetAsync(d_data.ptr() + len, 0, 64, stream));
  BlockTable T;
  T.upload(start, end, first, nb, n, device, stream);
  HIPCHK(hipStreamSynchronize(stream));      // (the sources are the caller's pageable memory)
  const float up_ms = t_up.ms();
  return split_and_decode(s, plain, d_data, len, T, start, end, first, nb, num_chunks, opts, stats, device, stream, up_ms, W);
}

// ---- deflate blocks on the device (inflate.hip) ------------------------------------------------------------------
static_assert(sizeof(rh_inflate_status) == sizeof(rhi::Status) && sizeof(rhi::Status) == 16, "rh_inflate_status is rhi::Status");
static_assert(RH_INFLATE_OK == rhi::ST_OK && RH_INFLATE_MALFORMED == rhi::ST_MALFORMED && RH_INFLATE_TRUNCATED == rhi::ST_TRUNCATED &&
              RH_INFLATE_TRAILING == rhi::ST_TRAILING && RH_INFLATE_TOO_LARGE == rhi::ST_TOO_LARGE && RH_INFLATE_INTERNAL == rhi::ST_INTERNAL, "status codes");

static constexpr uint64_t kBlockLimit = 0xFFFFFFF0ull;
static std::mutex g_inflate_last_mu;
static struct { float size_ms = 0, emit_ms = 0; uint64_t in_bytes = 0, out_bytes = 0; } g_inflate_last;

// one text per rule of inflate_core.h (DESIGN.md 14 lists them)
static const char* inflate_reason(const rhi::Status& s) {
  static const char* const which[3] = {"code-length", "literal/length", "distance"};
  static thread_local std::string buf;
  switch (s.reason) {
    case rhi::R_BLOCK_TYPE: return "block type 3";
    case rhi::R_STORED_LEN: return "a stored block's length and its complement do not match";
    case rhi::R_TOO_MANY: return "more than 286 literal/length or 30 distance symbols";
    case rhi::R_REPEAT: return "a length repeat with nothing to repeat, or past the last length";
    case rhi::R_NO_EOB: return "no code for end-of-block";
    case rhi::R_OVERSUBSCRIBED: buf = std::string("the ") + which[s.detail < 3 ? s.detail : 0] + " code is over-subscribed"; return buf.c_str();
    case rhi::R_INCOMPLETE: buf = std::string("the ") + which[s.detail < 3 ? s.detail : 0] + " code is incomplete"; return buf.c_str();
    case rhi::R_NO_CODE: buf = std::string("a ") + which[s.detail < 3 ? s.detail : 0] + " symbol that has no code"; return buf.c_str();
    case rhi::R_LITLEN_286: return "literal/length symbol 286 or 287";
    case rhi::R_DIST_30: return "distance symbol 30 or 31";
    case rhi::R_TOO_FAR: return "a distance further back than the bytes produced so far";
  }
  return "malformed stream";
}

static std::string inflate_message(uint64_t b, const rhi::Status& s) {
  const std::string where = block_where(b) + "deflate: ";
  switch (s.code) {
    case rhi::ST_MALFORMED: return where + inflate_reason(s);
    case rhi::ST_TRUNCATED: return where + "the stream ends before its final block";
    case rhi::ST_TRAILING: return where + std::to_string(s.detail) + " bytes behind the end of the stream";
    case rhi::ST_TOO_LARGE: return where + "it inflates to " + std::to_string(s.detail) + " bytes or more (a block of 4 GiB - 16 bytes or more is not supported)";
  }
  return where + "internal error";
}

// The two kernels around their one synchronisation.  size_pass: the compressed file and its table go up, sizes and verdicts come
// back.  The caller decides what a failing block means (and sets its size to 0 if it goes on), then emit_pass leases the
// output -- the accepted blocks back to back, no padding -- and fills it.
struct DeviceInflate {
  Lease d_comp, d_tab, d_out;
  std::vector<uint64_t> size, out_start;
  std::vector<rhi::Status> status;
  rh::InflateParams P;
  uint64_t nb = 0, in_bytes = 0, total = 0, o_out = 0;
  float size_ms = 0, emit_ms = 0;

  void size_pass(const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end, uint64_t nb_, uint64_t max_block, int device, hipStream_t stream) {
    nb = nb_;
    size.assign(nb, 0); out_start.assign(nb, 0); status.assign(nb, rhi::Status{0, 0, 0});
    d_comp = Lease(dev_pool(), len + 64, device);
    if (len) HIPCHK(hipMemcpyAsync(d_comp.ptr(), data, len, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemsetAsync(d_comp.ptr() + len, 0, 64, stream));
    // start[nb], end[nb], size[nb], out_start[nb], status[nb], emit_bad
    const uint64_t o_end = 8 * nb, o_size = 16 * nb, o_st = 32 * nb, o_bad = o_st + 16 * nb;
    o_out = 24 * nb;
    d_tab = Lease(dev_pool(), o_bad + 8, device);
    if (nb) {
      HIPCHK(hipMemcpyAsync(d_tab.ptr(), start, 8 * nb, hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(d_tab.ptr() + o_end, end, 8 * nb, hipMemcpyHostToDevice, stream));
    }
    HIPCHK(hipMemsetAsync(d_tab.ptr() + o_size, 0, o_bad + 8 - o_size, stream));
    std::memset(&P, 0, sizeof P);
    P.data = d_comp.ptr(); P.data_len = len;
    P.start = (const uint64_t*)d_tab.ptr(); P.end = (const uint64_t*)(d_tab.ptr() + o_end);
    P.nb = (uint32_t)nb; P.max_out = max_block;
    P.size = (uint64_t*)(d_tab.ptr() + o_size); P.out_start = (const uint64_t*)(d_tab.ptr() + o_out);
    P.status = (rhi::Status*)(d_tab.ptr() + o_st);
    P.emit_bad = (unsigned long long*)(d_tab.ptr() + o_bad);
    for (uint64_t b = 0; b < nb; b++) in_bytes += end[b] - start[b];
    Events ev;
    ev.init();
    ev.rec(0, stream);
    if (rh_launch_inflate_size(&P, stream)) throw HipError("k_inflate_size launch failed");
    ev.rec(1, stream);
    if (nb) {
      HIPCHK(hipMemcpyAsync(size.data(), P.size, 8 * nb, hipMemcpyDeviceToHost, stream));
      HIPCHK(hipMemcpyAsync(status.data(), P.status, 16 * nb, hipMemcpyDeviceToHost, stream));
    }
    HIPCHK(hipStreamSynchronize(stream));      // the one synchronisation: the host needs the total to lease the output
    size_ms = ev.ms(0, 1);
    for (uint64_t b = 0; b < nb; b++)
      if (status[b].code == rhi::ST_INTERNAL) throw std::runtime_error("internal error: the inflate size kernel refused the table of block " + std::to_string(b));
  }

  void emit_pass(int device, hipStream_t stream) {
    total = 0;
    for (uint64_t b = 0; b < nb; b++) {
      if (status[b].code != rhi::ST_OK) size[b] = 0;
      out_start[b] = total;
      total += size[b];
    }
    d_out = Lease(dev_pool(), total + 64, device);
    HIPCHK(hipMemsetAsync(d_out.ptr() + total, 0, 64, stream));
    if (nb) HIPCHK(hipMemcpyAsync(d_tab.ptr() + o_out, out_start.data(), 8 * nb, hipMemcpyHostToDevice, stream));
    P.out = d_out.ptr(); P.out_len = total;
    Events ev;
    ev.init();
    ev.rec(0, stream);
    if (rh_launch_inflate_emit(&P, stream)) throw HipError("k_inflate_emit launch failed");
    ev.rec(1, stream);
    unsigned long long bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, P.emit_bad, 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    emit_ms = ev.ms(0, 1);
    if (bad) throw std::runtime_error("internal error: the emit walk of deflate block " + std::to_string(~bad) + " disagrees with its size pass");
    d_comp.release();
    std::lock_guard<std::mutex> g(g_inflate_last_mu);
    g_inflate_last.size_ms = size_ms; g_inflate_last.emit_ms = emit_ms; g_inflate_last.in_bytes = in_bytes; g_inflate_last.out_bytes = total;
  }
};

static uint64_t block_limit_of(uint64_t max_block_bytes) { return max_block_bytes && max_block_bytes < kBlockLimit ? max_block_bytes : kBlockLimit; }

static void check_compressed_table(const uint64_t* start, const uint64_t* end, uint64_t nb, uint64_t len) {
  for (uint64_t b = 0; b < nb; b++)
    if (start[b] > end[b] || end[b] > len || (b && start[b] < end[b - 1])) throw std::invalid_argument(block_where(b) + "its bytes are outside the buffer or out of order");
}

// ---- deflate blocks written on the device (deflate.hip) ----------------------------------------------------------
static_assert(RH_DEFLATE_AUTO == rhd::AUTO && RH_DEFLATE_STORED == rhd::STORED && RH_DEFLATE_FIXED == rhd::FIXED && RH_DEFLATE_DYNAMIC == rhd::DYNAMIC,
              "RH_DEFLATE_* are the strategies of deflate_core.h");
static std::mutex g_deflate_last_mu;
static struct { float deflate_ms = 0, gather_ms = 0; uint64_t in_bytes = 0, out_bytes = 0; } g_deflate_last;

// What both deflate calls refuse before anything else.
static void check_deflate_call(const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end, uint64_t nb, uint32_t strategy) {
  if (nb > 0xFFFFFFFFull) throw std::invalid_argument("container: more than 2^32 - 1 blocks");
  if (nb && (!start || !end || !data)) throw std::invalid_argument("container: null block table");
  if (strategy > rhd::DYNAMIC) throw std::invalid_argument("container: deflate strategy " + std::to_string(strategy) + " is not one of 0 .. 3");
  check_compressed_table(start, end, nb, len);
  for (uint64_t b = 0; b < nb; b++)
    if (block_too_large(end[b] - start[b])) throw std::invalid_argument(block_large_message(b, end[b] - start[b]));
}

// The two kernels around their one synchronisation: the payloads and the segment table go up, rh_k_deflate fills the slots, the
// sizes come back and are prefix-summed here, rh_k_deflate_gather packs the streams, and the compressed bytes come down.
static void deflate_on_device(const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end, uint64_t nb, uint32_t strategy, int device,
                              hipStream_t stream, std::unique_ptr<uint8_t, void (*)(void*)>& host, uint64_t* out_len, uint64_t* out_start, uint64_t* out_end) {
  std::vector<uint64_t> seg_in, slot;
  std::vector<uint32_t> seg_len;
  uint64_t scratch_len = 0, in_bytes = 0;
  for (uint64_t b = 0; b < nb; b++) {
    const uint64_t size = end[b] - start[b], k = rhd::segments_of(size);
    in_bytes += size;
    for (uint64_t j = 0; j < k; j++) {
      const uint64_t at = j * rhd::kSegment, n = size - at < rhd::kSegment ? size - at : rhd::kSegment;
      const bool last = j + 1 == k;
      seg_in.push_back(start[b] + at);
      seg_len.push_back((uint32_t)n | (last ? rh::kSegLast : 0u));
      slot.push_back(scratch_len);
      scratch_len += (rhd::segment_bound(n, last) + 15) & ~15ull;
    }
  }
  const uint64_t ns = seg_in.size();
  if (ns > 0xFFFFFFFFull) throw std::invalid_argument("container: more than 2^32 - 1 deflate segments");
  Lease d_data(dev_pool(), len + 64, device), d_scratch(dev_pool(), scratch_len + 64, device);
  if (len) HIPCHK(hipMemcpyAsync(d_data.ptr(), data, len, hipMemcpyHostToDevice, stream));
  // seg_in[ns], slot[ns], out_at[ns], seg_len[ns], seg_size[ns], bad
  const uint64_t o_slot = 8 * ns, o_at = 16 * ns, o_len = 24 * ns, o_size = 28 * ns, o_bad = (32 * ns + 7) & ~7ull;
  Lease d_tab(dev_pool(), o_bad + 8, device);
  if (ns) {
    HIPCHK(hipMemcpyAsync(d_tab.ptr(), seg_in.data(), 8 * ns, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_tab.ptr() + o_slot, slot.data(), 8 * ns, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_tab.ptr() + o_len, seg_len.data(), 4 * ns, hipMemcpyHostToDevice, stream));
  }
  HIPCHK(hipMemsetAsync(d_tab.ptr() + o_size, 0, o_bad + 8 - o_size, stream));
  unsigned long long* d_bad = (unsigned long long*)(d_tab.ptr() + o_bad);
  rh::DeflateParams P;
  std::memset(&P, 0, sizeof P);
  P.data = d_data.ptr(); P.data_len = len;
  P.seg_in = (const uint64_t*)d_tab.ptr(); P.seg_len = (const uint32_t*)(d_tab.ptr() + o_len); P.slot = (const uint64_t*)(d_tab.ptr() + o_slot);
  P.scratch = d_scratch.ptr(); P.scratch_len = scratch_len;
  P.seg_size = (uint32_t*)(d_tab.ptr() + o_size);
  P.ns = (uint32_t)ns; P.strategy = strategy; P.bad = d_bad;
  Events ev;
  ev.init();
  ev.rec(0, stream);
  if (rh_launch_deflate(&P, stream)) throw HipError("k_deflate launch failed");
  ev.rec(1, stream);
  std::vector<uint32_t> seg_size(ns, 0);
  unsigned long long bad = 0;
  if (ns) HIPCHK(hipMemcpyAsync(seg_size.data(), P.seg_size, 4 * ns, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));      // the one synchronisation: the host needs the total to lease the output
  if (bad) throw std::runtime_error("internal error: the deflate kernel refused segment " + std::to_string(~bad));
  d_data.release();
  std::vector<uint64_t> out_at(ns, 0);
  uint64_t total = 0, s = 0;
  for (uint64_t b = 0; b < nb; b++) {
    out_start[b] = total;
    for (uint64_t k = rhd::segments_of(end[b] - start[b]); k; k--, s++) {
      out_at[s] = total;
      total += seg_size[s];
    }
    out_end[b] = total;
  }
  Lease d_out(dev_pool(), total + 64, device);
  if (ns) HIPCHK(hipMemcpyAsync(d_tab.ptr() + o_at, out_at.data(), 8 * ns, hipMemcpyHostToDevice, stream));
  rh::DeflateGatherParams G;
  std::memset(&G, 0, sizeof G);
  G.scratch = d_scratch.ptr(); G.scratch_len = scratch_len;
  G.slot = P.slot; G.seg_size = P.seg_size; G.out_at = (const uint64_t*)(d_tab.ptr() + o_at);
  G.out = d_out.ptr(); G.out_len = total; G.ns = (uint32_t)ns; G.bad = d_bad;
  ev.rec(2, stream);
  if (rh_launch_deflate_gather(&G, stream)) throw HipError("k_deflate_gather launch failed");
  ev.rec(3, stream);
  host.reset((uint8_t*)std::malloc(total ? total : 1));
  if (!host) throw std::bad_alloc();
  if (total) HIPCHK(hipMemcpyAsync(host.get(), d_out.ptr(), total, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  if (bad) throw std::runtime_error("internal error: the deflate gather kernel refused segment " + std::to_string(~bad));
  *out_len = total;
  std::lock_guard<std::mutex> g(g_deflate_last_mu);
  g_deflate_last.deflate_ms = ev.ms(0, 1); g_deflate_last.gather_ms = ev.ms(2, 3); g_deflate_last.in_bytes = in_bytes; g_deflate_last.out_bytes = total;
}

static rh_device_result* decode_cblocks_impl(rh_schema* s, const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end,
                                             const uint64_t* first, uint64_t nb, int codec, uint64_t max_block_bytes, uint64_t num_chunks,
                                             const rh_opts* opts, rh_stats* stats, WhereCall* W = nullptr) {
  if (codec == RH_CODEC_NULL) return decode_blocks_impl(s, data, len, start, end, first, nb, num_chunks, opts, stats, W);
  if (codec != RH_CODEC_DEFLATE) throw std::invalid_argument("container: codec must be RH_CODEC_NULL or RH_CODEC_DEFLATE");
  check_blocks_call(opts, data, start, end, first, nb);
  if (W) check_filter(s, W->f);
  rh_schema* const plain = plain_schema(s);
  const uint64_t min_rec = plain->cs->min_record_bytes;
  check_compressed_table(start, end, nb, len);
  for (uint64_t b = 0; b < nb; b++)
    if (first[b + 1] < first[b]) throw std::invalid_argument(block_where(b) + "negative record count");
  const uint64_t n = first[nb];
  check_empty_records(min_rec, n);

  require_device();
  int device = 0;
  if (opts && opts->device >= 0) { HIPCHK(hipSetDevice(opts->device)); device = opts->device; }
  else HIPCHK(hipGetDevice(&device));
  hipStream_t stream = opts ? (hipStream_t)opts->stream : nullptr;

  Timer t_up;
  DeviceInflate I;
  I.size_pass(data, len, start, end, nb, block_limit_of(max_block_bytes), device, stream);
  // deflate failures come before any record is walked, the lowest block first: as on the host road, which inflates every block first
  for (uint64_t b = 0; b < nb; b++)
    if (I.status[b].code != rhi::ST_OK) throw DecodeError(inflate_message(b, I.status[b]));
  std::vector<uint64_t> istart(nb), iend(nb);
  uint64_t at = 0;
  for (uint64_t b = 0; b < nb; b++) {
    check_block_size(b, I.size[b], first[b + 1] - first[b], min_rec);
    istart[b] = at;
    at += I.size[b];
    iend[b] = at;
  }
  I.emit_pass(device, stream);
  BlockTable T;
  T.upload(istart.data(), iend.data(), first, nb, n, device, stream);
  HIPCHK(hipStreamSynchronize(stream));      // (istart / iend are this frame's)
  const float up_ms = t_up.ms() - I.size_ms - I.emit_ms;
  return split_and_decode(s, plain, I.d_out, I.total, T, istart.data(), iend.data(), first, nb, num_chunks, opts, stats, device, stream, up_ms, W);
}

// ---- tolerant reads -------------------------------------------------------------------------------------------
static_assert(RH_BLOCK_END == rh::E_BLOCK_END, "RH_BLOCK_END is E_BLOCK_END");
static_assert(sizeof(rh::SalvageRec) == 32 && sizeof(rh::GatherJob) == 64, "device layouts");

static std::mutex g_salvage_last_mu;
static struct { float split_ms = 0, gather_ms = 0; uint64_t reported = 0, gathered = 0; } g_salvage_last;

static void note_salvage(float split_ms, float gather_ms, uint64_t reported, uint64_t gathered) {
  std::lock_guard<std::mutex> g(g_salvage_last_mu);
  g_salvage_last.split_ms = split_ms; g_salvage_last.gather_ms = gather_ms; g_salvage_last.reported = reported; g_salvage_last.gathered = gathered;
}

static std::string block_status_message(uint64_t b, const rh_block_status& st, uint64_t count) {
  if (st.code >= 1 && st.code < rh::E_BLOCK_END) {
    rh::ErrInfo ei; ei.code = st.code; ei.pad = 0; ei.detail = st.detail;
    return format_error(ei);
  }
  if (st.code == RH_BLOCK_END) return block_end_message(b, count, st.detail, st.aux);
  if (st.code == RH_BLOCK_COUNT) return block_count_message(b, count, (uint64_t)st.detail);
  if (st.code == RH_BLOCK_TOO_LARGE) return block_large_message(b, (uint64_t)st.detail);
  if (st.code > RH_BLOCK_INFLATE && st.code <= RH_BLOCK_INFLATE + rhi::ST_TOO_LARGE) {
    rhi::Status is; is.code = st.code - RH_BLOCK_INFLATE; is.reason = st.aux; is.detail = (uint64_t)st.detail;
    return inflate_message(b, is);
  }
  throw std::invalid_argument("container: a block status without a message");
}

// The tolerant road from "the bytes are on the device" onward.  start / end / first: the table the lanes walk -- a block that
// was dropped before the launch has an empty range and no record in it.  status[b].code != 0 marks those; `reported` counts
// them and the caller's own reports.  nullptr = more than max_errors reports.
static rh_device_result* salvage_and_decode(rh_schema* s, rh_schema* plain, Lease& d_data, uint64_t len, const std::vector<uint64_t>& start,
                                            const std::vector<uint64_t>& end, const std::vector<uint64_t>& first, uint64_t nb,
                                            rh_block_status* status, uint64_t reported, uint64_t extra_errors, uint64_t max_errors,
                                            uint64_t num_chunks, const rh_opts* opts, rh_stats* stats, int device, hipStream_t stream, float up_ms) {
  const uint64_t n = first[nb];
  BlockTable T;
  T.upload(start.data(), end.data(), first.data(), nb, n, device, stream);
  Lease d_rec(dev_pool(), sizeof(rh::SalvageRec) * std::max<uint64_t>(nb, 1), device);
  HIPCHK(hipStreamSynchronize(stream));      // (the table is the caller's frame's)
  float split_ms = 0;
  std::vector<rh::SalvageRec> recs;
  if (nb) {
    const DeviceProgram& dp = device_program(plain, device);
    rh::SalvageParams P;
    std::memset(&P, 0, sizeof P);
    rh::SParams& S = P.S;
    S.data = d_data.ptr(); S.data_len = len;
    S.start = (const uint64_t*)T.d_tab.ptr(); S.end = (const uint64_t*)(T.d_tab.ptr() + T.o_end); S.first = (const uint64_t*)(T.d_tab.ptr() + T.o_first);
    S.nb = (uint32_t)nb; S.list_depth = plain->cs->list_depth;
    S.prog = dp.prog; S.sym_off = dp.sym_off; S.sym_data = dp.sym_data;
    S.offsets = (uint64_t*)T.d_off.ptr();
    S.err = (rh::SplitErr*)(T.d_tab.ptr() + T.o_err);
    S.first_bad = (unsigned long long*)(T.d_tab.ptr() + T.o_bad);
    P.rec = (rh::SalvageRec*)d_rec.ptr();
    if (rh_split_lds_bytes(S.list_depth) > 160 * 1024 - 512) throw rh::SchemaError("schema needs more LDS than a CDNA4 workgroup has");
    Events ev;
    ev.init();
    ev.rec(0, stream);
    if (rh_launch_split_salvage(&P, stream)) throw HipError("k_split_salvage launch failed");
    ev.rec(1, stream);
    unsigned long long fb = 0;
    HIPCHK(hipMemcpyAsync(&fb, S.first_bad, 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    split_ms = ev.ms(0, 1);
    if (fb) {      // at least one lane stopped its block: what every lane left
      recs.resize(nb);
      HIPCHK(hipMemcpy(recs.data(), P.rec, sizeof(rh::SalvageRec) * nb, hipMemcpyDeviceToHost));
    }
  }
  g_split_last_ms.store(split_ms);
  for (uint64_t b = 0; b < nb; b++) {
    if (status[b].code) continue;      // (dropped before the launch: kept = 0)
    status[b].kept = first[b + 1] - first[b];
    if (recs.empty() || !recs[b].code) continue;
    const rh::SalvageRec& r = recs[b];
    if (r.kept > first[b + 1] - first[b] || r.kept_end < start[b] || r.kept_end > end[b])
      throw std::runtime_error("internal error: the salvage split left block " + std::to_string(b) + " a record outside its block");
    status[b].code = r.code; status[b].aux = r.code == rh::E_BLOCK_END ? (uint32_t)(end[b] - start[b]) : 0u;
    status[b].detail = r.detail; status[b].kept = r.kept;
    reported++;
  }
  if (reported > max_errors) {
    note_salvage(split_ms, 0, reported - extra_errors, 0);
    return nullptr;
  }

  if (!reported) {      // a clean file: the strict road's buffers as they are
    note_salvage(split_ms, 0, 0, 0);
    rh_device_result* r = decode_device_impl(s, d_data.ptr(), (const uint64_t*)T.d_off.ptr(), nb ? end[nb - 1] : 0, n, num_chunks, opts, stats);
    r->container_data = std::move(d_data);
    r->container_offsets = std::move(T.d_off);
    if (stats) stats->h2d_ms += up_ms;
    return r;
  }

  // gather_kept: the kept run of every block that keeps a record, each at the next multiple of 16, and the records renumbered
  std::vector<rh::GatherJob> jobs;
  uint64_t n2 = 0, at = 0;
  for (uint64_t b = 0; b < nb; b++) {
    const uint64_t kept = status[b].kept;
    if (!kept) continue;
    const uint64_t kept_end = !recs.empty() && recs[b].code ? recs[b].kept_end : end[b];
    rh::GatherJob j;
    j.src = start[b]; j.len = kept_end - start[b];
    j.dst = at; j.dst_next = align_up(at + j.len, 16);
    j.off_first = first[b]; j.new_first = n2; j.kept = kept; j.last = 0;
    jobs.push_back(j);
    n2 += kept;
    at = j.dst_next;
  }
  if (!jobs.empty()) jobs.back().last = 1;
  const uint64_t total = at, data_end = jobs.empty() ? 0 : jobs.back().dst + jobs.back().len;
  Lease d_out(dev_pool(), total + 64, device);
  Lease d_noff(dev_pool(), 8 * (n2 + 1), device);
  Lease d_jobs(dev_pool(), sizeof(rh::GatherJob) * std::max<size_t>(jobs.size(), 1), device);
  HIPCHK(hipMemsetAsync(d_out.ptr() + total, 0, 64, stream));
  if (jobs.empty()) HIPCHK(hipMemsetAsync(d_noff.ptr(), 0, 8, stream));      // (no wavefront: new_off[0] = 0)
  else HIPCHK(hipMemcpyAsync(d_jobs.ptr(), jobs.data(), sizeof(rh::GatherJob) * jobs.size(), hipMemcpyHostToDevice, stream));
  rh::SalvageGatherParams G;
  std::memset(&G, 0, sizeof G);
  G.data = d_data.ptr(); G.off = (const uint64_t*)T.d_off.ptr();
  G.jobs = (const rh::GatherJob*)d_jobs.ptr(); G.njobs = (uint32_t)jobs.size();
  G.out = d_out.ptr(); G.out_len = total; G.new_off = (uint64_t*)d_noff.ptr();
  Events ev;
  ev.init();
  ev.rec(0, stream);
  if (rh_launch_salvage_gather(&G, stream)) throw HipError("k_salvage_gather launch failed");
  ev.rec(1, stream);
  HIPCHK(hipStreamSynchronize(stream));      // (the jobs are this frame's; the split's buffers go back to the pool)
  note_salvage(split_ms, ev.ms(0, 1), reported - extra_errors, total);
  d_data.release();
  T.d_off.release();

  rh_device_result* r = decode_device_impl(s, d_out.ptr(), (const uint64_t*)d_noff.ptr(), data_end, n2, num_chunks, opts, stats);
  r->container_data = std::move(d_out);
  r->container_offsets = std::move(d_noff);
  if (stats) stats->h2d_ms += up_ms;
  return r;
}

static rh_device_result* decode_blocks_tolerant_impl(rh_schema* s, const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end,
                                                     const uint64_t* first, const uint8_t* dropped, uint64_t nb, int codec, uint64_t max_block_bytes,
                                                     uint64_t max_errors, uint64_t extra_errors, uint64_t num_chunks, const rh_opts* opts,
                                                     rh_block_status* status, rh_stats* stats) {
  if (codec != RH_CODEC_NULL && codec != RH_CODEC_DEFLATE) throw std::invalid_argument("container: codec must be RH_CODEC_NULL or RH_CODEC_DEFLATE");
  if (nb && !status) throw std::invalid_argument("container: null block status");
  check_blocks_call(opts, data, start, end, first, nb);
  rh_schema* const plain = plain_schema(s);
  const uint64_t min_rec = plain->cs->min_record_bytes;
  check_compressed_table(start, end, nb, len);
  for (uint64_t b = 0; b < nb; b++)
    if (first[b + 1] < first[b]) throw std::invalid_argument(block_where(b) + "negative record count");

  // the table the lanes walk: a block dropped here keeps its place with an empty range and no record
  std::vector<uint64_t> st(nb), en(nb), fi(nb + 1, 0);
  uint64_t reported = extra_errors;
  const auto drop = [&](uint64_t b, uint32_t code, uint32_t aux, int64_t detail) {
    status[b].code = code; status[b].aux = aux; status[b].detail = detail; status[b].kept = 0;
    reported++;
  };
  for (uint64_t b = 0; b < nb; b++) {
    status[b] = rh_block_status{0, 0, 0, 0};
    if (dropped && dropped[b]) drop(b, RH_BLOCK_DROPPED, 0, 0);
  }
  // the sizes of uncompressed blocks are known here: a file that cannot pass fails before any device work
  if (codec == RH_CODEC_NULL) {
    for (uint64_t b = 0; b < nb; b++) {
      const uint64_t size = end[b] - start[b], cnt = first[b + 1] - first[b];
      if (!status[b].code && block_too_large(size)) drop(b, RH_BLOCK_TOO_LARGE, 0, (int64_t)size);
      if (!status[b].code && block_count_refused(size, cnt, min_rec)) drop(b, RH_BLOCK_COUNT, 0, (int64_t)size);
      st[b] = start[b];
      en[b] = status[b].code ? start[b] : end[b];
      fi[b + 1] = fi[b] + (status[b].code ? 0 : cnt);
    }
    check_empty_records(min_rec, fi[nb]);
    if (reported > max_errors) return nullptr;
  }

  require_device();
  int device = 0;
  if (opts && opts->device >= 0) { HIPCHK(hipSetDevice(opts->device)); device = opts->device; }
  else HIPCHK(hipGetDevice(&device));
  hipStream_t stream = opts ? (hipStream_t)opts->stream : nullptr;

  Timer t_up;
  if (codec == RH_CODEC_NULL) {
    Lease d_data(dev_pool(), len + 64, device);
    if (len) HIPCHK(hipMemcpyAsync(d_data.ptr(), data, len, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemsetAsync(d_data.ptr() + len, 0, 64, stream));
    HIPCHK(hipStreamSynchronize(stream));      // (the source is the caller's pageable memory)
    const float up_ms = t_up.ms();
    return salvage_and_decode(s, plain, d_data, len, st, en, fi, nb, status, reported, extra_errors, max_errors, num_chunks, opts, stats, device, stream, up_ms);
  }

  // deflate: the size kernel's verdicts mark the refused streams; they inflate to nothing and hold no record
  std::vector<uint64_t> cend(end, end + nb);
  for (uint64_t b = 0; b < nb; b++)
    if (status[b].code) cend[b] = start[b];      // (a block the caller dropped: no stream to walk)
  DeviceInflate I;
  I.size_pass(data, len, start, cend.data(), nb, block_limit_of(max_block_bytes), device, stream);
  for (uint64_t b = 0; b < nb; b++) {
    if (status[b].code) { I.status[b].code = rhi::ST_TRUNCATED; continue; }      // (emit_pass gives it no byte)
    if (I.status[b].code != rhi::ST_OK) drop(b, RH_BLOCK_INFLATE + I.status[b].code, I.status[b].reason, (int64_t)I.status[b].detail);
  }
  uint64_t at = 0;
  for (uint64_t b = 0; b < nb; b++) {
    const uint64_t size = status[b].code ? 0 : I.size[b], cnt = first[b + 1] - first[b];
    if (!status[b].code && block_too_large(size)) drop(b, RH_BLOCK_TOO_LARGE, 0, (int64_t)size);
    if (!status[b].code && block_count_refused(size, cnt, min_rec)) drop(b, RH_BLOCK_COUNT, 0, (int64_t)size);
    st[b] = at;
    en[b] = status[b].code ? at : at + size;      // (a block refused for its count is inflated and then not walked)
    fi[b + 1] = fi[b] + (status[b].code ? 0 : cnt);
    at += size;
  }
  check_empty_records(min_rec, fi[nb]);
  if (reported > max_errors) return nullptr;
  I.emit_pass(device, stream);
  const float up_ms = t_up.ms() - I.size_ms - I.emit_ms;
  return salvage_and_decode(s, plain, I.d_out, I.total, st, en, fi, nb, status, reported, extra_errors, max_errors, num_chunks, opts, stats, device, stream, up_ms);
}

}  // namespace rhe

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

int rh_container_scan(const uint8_t* data, uint64_t len, rh_container_info** info, char** err) {
  if (!info) return RH_ERR_ARGUMENT;
  *info = nullptr;
  return guarded(err, [&] {
    std::unique_ptr<rh_container_info> ci(new rh_container_info);
    const std::string msg = rhc::container_scan(data, len, ci->ci);
    if (!msg.empty()) throw DecodeError(msg);
    *info = ci.release();
    return RH_OK;
  });
}

const char* rh_container_info_schema(const rh_container_info* i, uint64_t* len) {
  if (!i) return nullptr;
  if (len) *len = i->ci.schema.size();
  return i->ci.schema.c_str();
}
const char* rh_container_info_codec(const rh_container_info* i) { return i ? i->ci.codec.c_str() : nullptr; }
const uint8_t* rh_container_info_sync(const rh_container_info* i) { return i ? i->ci.sync : nullptr; }
uint64_t rh_container_info_blocks(const rh_container_info* i) { return i ? i->ci.nb() : 0; }
uint64_t rh_container_info_records(const rh_container_info* i) { return i ? i->ci.n() : 0; }
int rh_container_info_table(const rh_container_info* i, const uint64_t** start, const uint64_t** end, const uint64_t** first) {
  if (!i) return RH_ERR_ARGUMENT;
  if (start) *start = i->ci.start.data();
  if (end) *end = i->ci.end.data();
  if (first) *first = i->ci.first.data();
  return RH_OK;
}
uint32_t rh_container_info_metadata_count(const rh_container_info* i) { return i ? (uint32_t)i->ci.metadata.size() : 0; }
int rh_container_info_metadata_get(const rh_container_info* i, uint32_t k, const char** key, const uint8_t** value, uint64_t* value_len) {
  if (!i || k >= i->ci.metadata.size()) return RH_ERR_ARGUMENT;
  if (key) *key = i->ci.metadata[k].first.c_str();
  if (value) *value = (const uint8_t*)i->ci.metadata[k].second.data();
  if (value_len) *value_len = i->ci.metadata[k].second.size();
  return RH_OK;
}
void rh_container_info_free(rh_container_info* i) { delete i; }

int rh_container_salvage(const uint8_t* data, uint64_t len, rh_container_info** info, char** err) {
  if (!info) return RH_ERR_ARGUMENT;
  *info = nullptr;
  return guarded(err, [&] {
    std::unique_ptr<rh_container_info> ci(new rh_container_info);
    const std::string msg = rhc::container_salvage(data, len, ci->sv);
    if (!msg.empty()) throw DecodeError(msg);
    ci->ci = std::move(ci->sv.info);
    ci->salvaged = true;
    *info = ci.release();
    return RH_OK;
  });
}

int rh_container_info_salvage(const rh_container_info* i, uint64_t* header_end, const uint64_t** header_offset, const uint64_t** count,
                              const uint8_t** refused, uint64_t* gaps, uint64_t* steps) {
  if (!i || !i->salvaged) return RH_ERR_ARGUMENT;
  if (header_end) *header_end = i->sv.header_end;
  if (header_offset) *header_offset = i->sv.header_offset.data();
  if (count) *count = i->sv.count.data();
  if (refused) *refused = i->sv.refused.data();
  if (gaps) *gaps = i->sv.gaps.size();
  if (steps) *steps = i->sv.steps;
  return RH_OK;
}

int rh_container_info_gap(const rh_container_info* i, uint64_t k, uint64_t* offset, uint64_t* length, uint64_t* block, const char** message) {
  if (!i || !i->salvaged || k >= i->sv.gaps.size()) return RH_ERR_ARGUMENT;
  const rhc::SalvageInfo::Gap& g = i->sv.gaps[k];
  if (offset) *offset = g.offset;
  if (length) *length = g.length;
  if (block) *block = g.block;
  if (message) *message = g.message.c_str();
  return RH_OK;
}

int rh_block_status_message(uint64_t block, const rh_block_status* status, uint64_t count, char** message) {
  if (!status || !message) return RH_ERR_ARGUMENT;
  *message = nullptr;
  return guarded(message, [&] {
    *message = dup_msg(block_status_message(block, *status, count));
    return RH_OK;
  });
}

int rh_decode_blocks_tolerant_device(const rh_schema* s, const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end,
                                     const uint64_t* first, const uint8_t* dropped, uint64_t nb, int codec, uint64_t max_block_bytes,
                                     uint64_t max_errors, uint64_t extra_errors, uint64_t num_chunks, const rh_opts* opts,
                                     rh_device_result** out, rh_block_status* status, int* too_many, rh_stats* stats, char** err) {
  if (!s || !out || !too_many) return RH_ERR_ARGUMENT;
  *out = nullptr;
  *too_many = 0;
  return guarded(err, [&] {
    Timer t;
    rh_opts pub;
    if (opts) { pub = *opts; pub.flags &= kPublicFlags; }
    *out = decode_blocks_tolerant_impl(const_cast<rh_schema*>(s), data, len, start, end, first, dropped, nb, codec, max_block_bytes, max_errors,
                                       extra_errors, num_chunks, opts ? &pub : nullptr, status, stats);
    if (!*out) *too_many = 1;
    if (stats) stats->total_ms = t.ms();
    return RH_OK;
  });
}

int rh_decode_blocks_tolerant(const rh_schema* s, const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end,
                              const uint64_t* first, const uint8_t* dropped, uint64_t nb, int codec, uint64_t max_block_bytes,
                              uint64_t max_errors, uint64_t extra_errors, uint64_t num_chunks, const rh_opts* opts,
                              struct ArrowArray* out_chunks, uint32_t out_cap, uint32_t* out_k, rh_block_status* status, int* too_many,
                              rh_stats* stats, char** err) {
  if (!s || !out_chunks || !too_many) return RH_ERR_ARGUMENT;
  *too_many = 0;
  if (out_k) *out_k = 0;
  return guarded(err, [&] {
    Timer t;
    rh_opts pub;
    if (opts) { pub = *opts; pub.flags &= kPublicFlags; }
    std::unique_ptr<rh_device_result> r(decode_blocks_tolerant_impl(const_cast<rh_schema*>(s), data, len, start, end, first, dropped, nb, codec,
                                                                    max_block_bytes, max_errors, extra_errors, num_chunks, opts ? &pub : nullptr,
                                                                    status, stats));
    if (!r) { *too_many = 1; return (int)RH_OK; }
    if (r->k > out_cap) throw std::invalid_argument("container: out_chunks has room for " + std::to_string(out_cap) + " chunks, the call made " + std::to_string(r->k));
    Timer td;
    const int rc = to_host_impl(r.get(), out_chunks, opts ? (hipStream_t)opts->stream : nullptr);
    if (stats) stats->d2h_ms = td.ms();
    if (out_k) *out_k = r->k;
    if (stats) stats->total_ms = t.ms();
    return rc;
  });
}

void rh_salvage_last(float* split_ms, float* gather_ms, uint64_t* blocks_reported, uint64_t* bytes_gathered) {
  std::lock_guard<std::mutex> g(g_salvage_last_mu);
  if (split_ms) *split_ms = g_salvage_last.split_ms;
  if (gather_ms) *gather_ms = g_salvage_last.gather_ms;
  if (blocks_reported) *blocks_reported = g_salvage_last.reported;
  if (bytes_gathered) *bytes_gathered = g_salvage_last.gathered;
}

float rh_split_last_ms(void) { return g_split_last_ms.load(); }

int rh_decode_blocks_device(const rh_schema* s, const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end,
                            const uint64_t* first, uint64_t nb, uint64_t num_chunks, const rh_opts* opts, rh_device_result** out,
                            rh_stats* stats, char** err) {
  if (!s || !out) return RH_ERR_ARGUMENT;
  *out = nullptr;
  return guarded(err, [&] {
    Timer t;
    rh_opts pub;
    if (opts) { pub = *opts; pub.flags &= kPublicFlags; }
    *out = decode_blocks_impl(const_cast<rh_schema*>(s), data, len, start, end, first, nb, num_chunks, opts ? &pub : nullptr, stats);
    if (stats) stats->total_ms = t.ms();
    return RH_OK;
  });
}

int rh_decode_blocks(const rh_schema* s, const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end,
                     const uint64_t* first, uint64_t nb, uint64_t num_chunks, const rh_opts* opts, struct ArrowArray* out_chunks,
                     uint32_t* out_k, rh_stats* stats, char** err) {
  if (!s || !out_chunks) return RH_ERR_ARGUMENT;
  return guarded(err, [&] {
    Timer t;
    rh_opts pub;
    if (opts) { pub = *opts; pub.flags &= kPublicFlags; }
    std::unique_ptr<rh_device_result> r(
        decode_blocks_impl(const_cast<rh_schema*>(s), data, len, start, end, first, nb, num_chunks, opts ? &pub : nullptr, stats));
    Timer td;
    const int rc = to_host_impl(r.get(), out_chunks, opts ? (hipStream_t)opts->stream : nullptr);
    if (stats) stats->d2h_ms = td.ms();
    if (out_k) *out_k = r->k;
    if (stats) stats->total_ms = t.ms();
    return rc;
  });
}

int rh_decode_cblocks_device(const rh_schema* s, const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end,
                             const uint64_t* first, uint64_t nb, int codec, uint64_t max_block_bytes, uint64_t num_chunks,
                             const rh_opts* opts, rh_device_result** out, rh_stats* stats, char** err) {
  if (!s || !out) return RH_ERR_ARGUMENT;
  *out = nullptr;
  return guarded(err, [&] {
    Timer t;
    rh_opts pub;
    if (opts) { pub = *opts; pub.flags &= kPublicFlags; }
    *out = decode_cblocks_impl(const_cast<rh_schema*>(s), data, len, start, end, first, nb, codec, max_block_bytes, num_chunks,
                               opts ? &pub : nullptr, stats);
    if (stats) stats->total_ms = t.ms();
    return RH_OK;
  });
}

int rh_decode_cblocks(const rh_schema* s, const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end,
                      const uint64_t* first, uint64_t nb, int codec, uint64_t max_block_bytes, uint64_t num_chunks, const rh_opts* opts,
                      struct ArrowArray* out_chunks, uint32_t* out_k, rh_stats* stats, char** err) {
  if (!s || !out_chunks) return RH_ERR_ARGUMENT;
  return guarded(err, [&] {
    Timer t;
    rh_opts pub;
    if (opts) { pub = *opts; pub.flags &= kPublicFlags; }
    std::unique_ptr<rh_device_result> r(decode_cblocks_impl(const_cast<rh_schema*>(s), data, len, start, end, first, nb, codec, max_block_bytes,
                                                            num_chunks, opts ? &pub : nullptr, stats));
    Timer td;
    const int rc = to_host_impl(r.get(), out_chunks, opts ? (hipStream_t)opts->stream : nullptr);
    if (stats) stats->d2h_ms = td.ms();
    if (out_k) *out_k = r->k;
    if (stats) stats->total_ms = t.ms();
    return rc;
  });
}

// ---- row filters in the split walk ------------------------------------------------------------------------------
int rh_decode_cblocks_device_where(const rh_schema* s, const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end,
                                   const uint64_t* first, uint64_t nb, int codec, uint64_t max_block_bytes, uint64_t num_chunks,
                                   const rh_opts* opts, rh_device_result** out, rh_stats* stats, char** err, const rh_filter* filter,
                                   uint64_t* kept) {
  if (!s || !out || !filter) return RH_ERR_ARGUMENT;
  *out = nullptr;
  return guarded(err, [&] {
    Timer t;
    rh_opts pub;
    if (opts) { pub = *opts; pub.flags &= kPublicFlags; }
    WhereCall W;
    W.f = const_cast<rh_filter*>(filter);
    *out = decode_cblocks_impl(const_cast<rh_schema*>(s), data, len, start, end, first, nb, codec, max_block_bytes, num_chunks,
                               opts ? &pub : nullptr, stats, &W);
    if (kept) *kept = W.kept;
    if (stats) stats->total_ms = t.ms();
    return RH_OK;
  });
}

int rh_decode_cblocks_where(const rh_schema* s, const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end,
                            const uint64_t* first, uint64_t nb, int codec, uint64_t max_block_bytes, uint64_t num_chunks, const rh_opts* opts,
                            struct ArrowArray* out_chunks, uint32_t* out_k, rh_stats* stats, char** err, const rh_filter* filter,
                            uint64_t* kept) {
  if (!s || !out_chunks || !filter) return RH_ERR_ARGUMENT;
  return guarded(err, [&] {
    Timer t;
    rh_opts pub;
    if (opts) { pub = *opts; pub.flags &= kPublicFlags; }
    WhereCall W;
    W.f = const_cast<rh_filter*>(filter);
    std::unique_ptr<rh_device_result> r(decode_cblocks_impl(const_cast<rh_schema*>(s), data, len, start, end, first, nb, codec, max_block_bytes,
                                                            num_chunks, opts ? &pub : nullptr, stats, &W));
    if (kept) *kept = W.kept;
    Timer td;
    const int rc = to_host_impl(r.get(), out_chunks, opts ? (hipStream_t)opts->stream : nullptr);
    if (stats) stats->d2h_ms = td.ms();
    if (out_k) *out_k = r->k;
    if (stats) stats->total_ms = t.ms();
    return rc;
  });
}

int rh_decode_blocks_device_where(const rh_schema* s, const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end,
                                  const uint64_t* first, uint64_t nb, uint64_t num_chunks, const rh_opts* opts, rh_device_result** out,
                                  rh_stats* stats, char** err, const rh_filter* filter, uint64_t* kept) {
  return rh_decode_cblocks_device_where(s, data, len, start, end, first, nb, RH_CODEC_NULL, 0, num_chunks, opts, out, stats, err, filter, kept);
}

int rh_decode_blocks_where(const rh_schema* s, const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end,
                           const uint64_t* first, uint64_t nb, uint64_t num_chunks, const rh_opts* opts, struct ArrowArray* out_chunks,
                           uint32_t* out_k, rh_stats* stats, char** err, const rh_filter* filter, uint64_t* kept) {
  return rh_decode_cblocks_where(s, data, len, start, end, first, nb, RH_CODEC_NULL, 0, num_chunks, opts, out_chunks, out_k, stats, err, filter,
                                 kept);
}

int rh_filter_cblocks(const rh_filter* f, const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end, const uint64_t* first,
                      uint64_t nb, int codec, uint64_t max_block_bytes, const rh_opts* opts, uint64_t* keep_words, uint64_t* kept, char** err) {
  if (!f) return RH_ERR_ARGUMENT;
  return guarded(err, [&] {
    rh_opts pub;
    if (opts) { pub = *opts; pub.flags &= kPublicFlags; }
    WhereCall W;
    W.f = const_cast<rh_filter*>(f);
    W.mask_only = true;
    W.keep_words = keep_words;
    decode_cblocks_impl(f->plain, data, len, start, end, first, nb, codec, max_block_bytes, 1, opts ? &pub : nullptr, nullptr, &W);
    if (kept) *kept = W.kept;
    return RH_OK;
  });
}

int rh_filter_blocks(const rh_filter* f, const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end, const uint64_t* first,
                     uint64_t nb, const rh_opts* opts, uint64_t* keep_words, uint64_t* kept, char** err) {
  return rh_filter_cblocks(f, data, len, start, end, first, nb, RH_CODEC_NULL, 0, opts, keep_words, kept, err);
}

void rh_container_where_last(float* split_ms, float* gather_ms, uint64_t* n, uint64_t* kept) {
  std::lock_guard<std::mutex> g(g_where_last_mu);
  if (split_ms) *split_ms = g_where_last.split_ms;
  if (gather_ms) *gather_ms = g_where_last.gather_ms;
  if (n) *n = g_where_last.n;
  if (kept) *kept = g_where_last.kept;
}

int rh_inflate_blocks(const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end, uint64_t nb, uint64_t max_block_bytes,
                      const rh_opts* opts, uint8_t** out, uint64_t* out_len, uint64_t* out_start, uint64_t* out_end,
                      rh_inflate_status* status, char** err) {
  if (!out || !out_len || (nb && (!out_start || !out_end || !status))) return RH_ERR_ARGUMENT;
  *out = nullptr;
  *out_len = 0;
  return guarded(err, [&] {
    if (opts && opts->n_devices > 0) throw std::invalid_argument("container: a container is read on one device (rh_opts.devices is refused)");
    if (opts && (opts->flags & RH_ASYNC)) throw std::invalid_argument("container: the blocks call is synchronous: RH_ASYNC is refused");
    if (nb > 0xFFFFFFFFull) throw std::invalid_argument("container: more than 2^32 - 1 blocks");
    if (nb && (!start || !end || !data)) throw std::invalid_argument("container: null block table");
    check_compressed_table(start, end, nb, len);
    require_device();
    int device = 0;
    if (opts && opts->device >= 0) { HIPCHK(hipSetDevice(opts->device)); device = opts->device; }
    else HIPCHK(hipGetDevice(&device));
    hipStream_t stream = opts ? (hipStream_t)opts->stream : nullptr;
    DeviceInflate I;
    I.size_pass(data, len, start, end, nb, block_limit_of(max_block_bytes), device, stream);
    I.emit_pass(device, stream);      // (a failing block contributes no byte)
    std::unique_ptr<uint8_t, void (*)(void*)> host((uint8_t*)std::malloc(I.total ? I.total : 1), std::free);
    if (!host) throw std::bad_alloc();
    if (I.total) HIPCHK(hipMemcpyAsync(host.get(), I.d_out.ptr(), I.total, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    for (uint64_t b = 0; b < nb; b++) {
      out_start[b] = I.out_start[b];
      out_end[b] = I.out_start[b] + I.size[b];
      status[b].code = I.status[b].code; status[b].reason = I.status[b].reason; status[b].detail = I.status[b].detail;
    }
    *out = host.release();
    *out_len = I.total;
    return RH_OK;
  });
}

void rh_inflate_last(float* size_ms, float* emit_ms, uint64_t* in_bytes, uint64_t* out_bytes) {
  std::lock_guard<std::mutex> g(g_inflate_last_mu);
  if (size_ms) *size_ms = g_inflate_last.size_ms;
  if (emit_ms) *emit_ms = g_inflate_last.emit_ms;
  if (in_bytes) *in_bytes = g_inflate_last.in_bytes;
  if (out_bytes) *out_bytes = g_inflate_last.out_bytes;
}

int rh_deflate_blocks(const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end, uint64_t nb, uint32_t strategy,
                      const rh_opts* opts, uint8_t** out, uint64_t* out_len, uint64_t* out_start, uint64_t* out_end, char** err) {
  if (!out || !out_len || (nb && (!out_start || !out_end))) return RH_ERR_ARGUMENT;
  *out = nullptr;
  *out_len = 0;
  return guarded(err, [&] {
    if (opts && opts->n_devices > 0) throw std::invalid_argument("container: a container is written on one device (rh_opts.devices is refused)");
    if (opts && (opts->flags & RH_ASYNC)) throw std::invalid_argument("container: the blocks call is synchronous: RH_ASYNC is refused");
    check_deflate_call(data, len, start, end, nb, strategy);
    require_device();
    int device = 0;
    if (opts && opts->device >= 0) { HIPCHK(hipSetDevice(opts->device)); device = opts->device; }
    else HIPCHK(hipGetDevice(&device));
    hipStream_t stream = opts ? (hipStream_t)opts->stream : nullptr;
    std::unique_ptr<uint8_t, void (*)(void*)> host(nullptr, std::free);
    deflate_on_device(data, len, start, end, nb, strategy, device, stream, host, out_len, out_start, out_end);
    *out = host.release();
    return RH_OK;
  });
}

int rh_deflate_blocks_host(const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end, uint64_t nb, uint32_t strategy,
                           uint8_t** out, uint64_t* out_len, uint64_t* out_start, uint64_t* out_end, char** err) {
  if (!out || !out_len || (nb && (!out_start || !out_end))) return RH_ERR_ARGUMENT;
  *out = nullptr;
  *out_len = 0;
  return guarded(err, [&] {
    check_deflate_call(data, len, start, end, nb, strategy);
    uint64_t room = 0;
    for (uint64_t b = 0; b < nb; b++) room += rhd::deflate_bound(end[b] - start[b]);
    std::unique_ptr<uint8_t, void (*)(void*)> host((uint8_t*)std::malloc(room ? room : 1), std::free);
    if (!host) throw std::bad_alloc();
    std::unique_ptr<rhd::State> S(new rhd::State);
    uint64_t total = 0;
    for (uint64_t b = 0; b < nb; b++) {
      const uint64_t size = rhd::deflate_stream_host(*S, data + start[b], end[b] - start[b], strategy, host.get() + total);
      if (size == ~0ull) throw std::runtime_error("internal error: the deflate writer passed the bound of block " + std::to_string(b));
      out_start[b] = total;
      total += size;
      out_end[b] = total;
    }
    *out = host.release();
    *out_len = total;
    return RH_OK;
  });
}

uint64_t rh_deflate_bound(uint64_t len) { return rhd::deflate_bound(len); }

void rh_deflate_last(float* deflate_ms, float* gather_ms, uint64_t* in_bytes, uint64_t* out_bytes) {
  std::lock_guard<std::mutex> g(g_deflate_last_mu);
  if (deflate_ms) *deflate_ms = g_deflate_last.deflate_ms;
  if (gather_ms) *gather_ms = g_deflate_last.gather_ms;
  if (in_bytes) *in_bytes = g_deflate_last.in_bytes;
  if (out_bytes) *out_bytes = g_deflate_last.out_bytes;
}

}  // extern "C"
