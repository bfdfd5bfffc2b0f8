// Avro object container files: the framing scan behind the C ABI (rh_container_scan: host only) and the
// blocks entry points (rh_decode_blocks / rh_decode_blocks_device): the file uploaded as it is, rh_k_split (container.hip)
// turning the block table into record offsets, then the device-input decode (decode_device_impl) on (d_data, d_offsets, n).
#include "engine_internal.h"
#include "container.h"
#include "container_scan.h"

extern "C" {
uint32_t rh_split_lds_bytes(int list_depth);
int rh_launch_split(const rh::SParams* S, void* stream);
}

using namespace rhe;

struct rh_container_info {
  rhc::ContainerInfo ci;
};

namespace rhe {

static std::atomic<float> g_split_last_ms{0.0f};
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

static rh_device_result* decode_blocks_impl(rh_schema* s, const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end,
                                            const uint64_t* first, uint64_t nb, uint64_t num_chunks, const rh_opts* opts, rh_stats* stats) {
  if (opts && opts->n_devices > 0) throw std::invalid_argument("container: a container is read on one device (rh_opts.devices is refused)");
  if (opts && (opts->flags & RH_ASYNC)) throw std::invalid_argument("container: the blocks call is synchronous: RH_ASYNC is refused");
  if (opts && opts->chunk_rows) throw std::invalid_argument("container: chunk_rows applies to rh_decode_device only");
  if (nb > 0xFFFFFFFFull) throw std::invalid_argument("container: more than 2^32 - 1 blocks");
  if (nb && (!start || !end || !data)) throw std::invalid_argument("container: null block table");
  if (!first || first[0] != 0) throw std::invalid_argument("container: first[0] must be 0");
  rh_schema* const plain = plain_schema(s);
  const uint64_t min_rec = plain->cs->min_record_bytes;
  for (uint64_t b = 0; b < nb; b++) {
    const auto where = [b] { return "container: block " + std::to_string(b) + ": "; };      // (error paths only)
    if (start[b] > end[b] || end[b] > len || (b && start[b] < end[b - 1])) throw std::invalid_argument(where() + "its bytes are outside the buffer or out of order");
    if (first[b + 1] < first[b]) throw std::invalid_argument(where() + "negative record count");
    const uint64_t size = end[b] - start[b], cnt = first[b + 1] - first[b];
    if (size >= 0xFFFFFFF0ull) throw DecodeError(where() + "a block of 4 GiB - 16 bytes or more is not supported (" + std::to_string(size) + " bytes)");
    // what bounds a lane's loop, and through it the call's records and its offsets: every record has its minimum wire bytes
    if (min_rec && cnt > size / min_rec)
      throw DecodeError(where() + std::to_string(cnt) + " records cannot be in its " + std::to_string(size) + " bytes");
  }
  const uint64_t n = first[nb];
  // records of no bytes at all (a schema of empty records) are bounded by no byte count: by a count for the whole call, which
  // bounds every block's loop too -- a small file of many such blocks may not size the offsets
  if (!min_rec && n > kMaxEmptyRecords)
    throw DecodeError("container: " + std::to_string(n) + " records of a schema whose records may be empty: at most " +
                      std::to_string(kMaxEmptyRecords) + " in one call");

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
  Lease d_off(dev_pool(), 8 * (n + 1), device);
  const uint64_t o_end = 8 * nb, o_first = 16 * nb, o_err = align_up(o_first + 8 * (nb + 1), 16), o_bad = o_err + sizeof(rh::SplitErr) * nb;
  Lease d_tab(dev_pool(), o_bad + 8, device);
  if (nb) {
    HIPCHK(hipMemcpyAsync(d_tab.ptr(), start, 8 * nb, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_tab.ptr() + o_end, end, 8 * nb, hipMemcpyHostToDevice, stream));
  }
  HIPCHK(hipMemcpyAsync(d_tab.ptr() + o_first, first, 8 * (nb + 1), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemsetAsync(d_tab.ptr() + o_err, 0, o_bad + 8 - o_err, stream));
  const uint64_t data_end = nb ? end[nb - 1] : 0;
  if (nb == 0) HIPCHK(hipMemsetAsync(d_off.ptr(), 0, 8, stream));      // (no block, no lane: offsets[0] = 0)
  HIPCHK(hipStreamSynchronize(stream));      // (the sources are the caller's pageable memory)
  const float up_ms = t_up.ms();

  float split_ms = 0;
  if (nb) {
    const DeviceProgram& dp = device_program(plain, device);
    rh::SParams S;
    std::memset(&S, 0, sizeof S);
    S.data = d_data.ptr(); S.data_len = len;
    S.start = (const uint64_t*)d_tab.ptr(); S.end = (const uint64_t*)(d_tab.ptr() + o_end); S.first = (const uint64_t*)(d_tab.ptr() + o_first);
    S.nb = (uint32_t)nb; S.list_depth = plain->cs->list_depth;
    S.prog = dp.prog; S.sym_off = dp.sym_off; S.sym_data = dp.sym_data;
    S.offsets = (uint64_t*)d_off.ptr();
    S.err = (rh::SplitErr*)(d_tab.ptr() + o_err);
    S.first_bad = (unsigned long long*)(d_tab.ptr() + o_bad);
    if (rh_split_lds_bytes(S.list_depth) > 160 * 1024 - 512) throw rh::SchemaError("schema needs more LDS than a CDNA4 workgroup has");
    Events ev;
    ev.init();
    ev.rec(0, stream);
    if (rh_launch_split(&S, stream)) throw HipError("k_split launch failed");
    ev.rec(1, stream);
    unsigned long long fb = 0;
    HIPCHK(hipMemcpyAsync(&fb, S.first_bad, 8, hipMemcpyDeviceToHost, stream));
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
          throw DecodeError("container: block " + std::to_string(b) + ": its " + std::to_string(first[b + 1] - first[b]) + " records end at byte " +
                            std::to_string(errs[b].detail) + " of " + std::to_string(end[b] - start[b]));
      throw std::runtime_error("internal error: the split kernel reported a failure no block owns");
    }
  }
  g_split_last_ms.store(split_ms);

  rh_device_result* r = decode_device_impl(s, d_data.ptr(), (const uint64_t*)d_off.ptr(), data_end, n, num_chunks, opts, stats);
  r->container_data = std::move(d_data);      // the result owns every byte its call read (as a repaired tolerant call's)
  r->container_offsets = std::move(d_off);
  if (stats) stats->h2d_ms += up_ms;
  return r;
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

}  // extern "C"
