// Tolerant decode (DESIGN.md "Tolerant decode"): the placeholder datum of a schema, the validation of a call's records
// (rh_validate*: ALL malformed records, not the lowest one) and the optimistic repair around the strict decode calls
// (rh_decode*_tolerant): the strict call as it is; only when it fails on a record, one validation pass, the malformed
// records replaced by the placeholder, and the strict call again.  A clean call launches, allocates and copies nothing
// beyond what the strict call does.
#include "engine_internal.h"
#include "validate.h"

extern "C" {
uint32_t rh_validate_lds_fixed(int list_depth);
int rh_launch_validate(const rh::VParams* V, uint32_t lds_bytes, void* stream);
int rh_launch_patch_offsets(const rh::GParams* G, void* stream);
int rh_launch_patch_gather(const rh::GParams* G, void* stream);
}

using namespace rhe;

struct rh_record_errors {
  std::vector<uint64_t> index;
  std::vector<int> code;
  std::vector<std::string> message;
};

namespace rhe {

// ---------------------------------------------------------------------------
// the placeholder datum: the shortest datum of the schema that the strict decoder accepts
// ---------------------------------------------------------------------------
static void put_long(std::vector<uint8_t>& o, int64_t v) {
  uint64_t z = ((uint64_t)v << 1) ^ (uint64_t)(v >> 63);
  while (z >= 0x80) { o.push_back((uint8_t)(z | 0x80)); z >>= 7; }
  o.push_back((uint8_t)z);
}

static void placeholder_of(const rh::AvroType& t, std::vector<uint8_t>& o) {
  switch (t.kind) {
    case rh::AV_NULL: break;
    case rh::AV_FLOAT: o.insert(o.end(), 4, 0); break;
    case rh::AV_DOUBLE: o.insert(o.end(), 8, 0); break;
    case rh::AV_FIXED: o.insert(o.end(), (size_t)std::max<int64_t>(t.size, 0), 0); break;
    case rh::AV_DURATION: o.insert(o.end(), 12, 0); break;
    case rh::AV_UUID:
      if (t.size >= 0) { o.insert(o.end(), (size_t)t.size, 0); break; }
      put_long(o, 36);                                   // on a string: the nil uuid (an empty string is no uuid)
      for (const char* p = "00000000-0000-0000-0000-000000000000"; *p; p++) o.push_back((uint8_t)*p);
      break;
    case rh::AV_DECIMAL:
      if (t.size >= 0) o.insert(o.end(), (size_t)t.size, 0);
      else { o.push_back(0x02); o.push_back(0x00); }     // on bytes: one byte, the value 0
      break;
    case rh::AV_RECORD:
      for (const rh::AvroField& f : t.fields) placeholder_of(*f.type, o);
      break;
    case rh::AV_UNION: {
      for (size_t i = 0; i < t.variants.size(); i++)
        if (t.variants[i]->kind == rh::AV_NULL) { put_long(o, (int64_t)i); return; }
      put_long(o, 0);
      if (!t.variants.empty()) placeholder_of(*t.variants[0], o);
      break;
    }
    case rh::AV_REF: throw rh::SchemaError("placeholder: unresolved named-type reference " + t.fullname());
    default: o.push_back(0); break;      // boolean, int / long and the logical types over them, enum, string / bytes, array / map
  }
}

const std::vector<uint8_t>& placeholder_datum(rh_schema* s) {
  std::lock_guard<std::mutex> g(s->mu);
  if (!s->placeholder_done) {
    std::vector<uint8_t> o;
    placeholder_of(*s->cs->avro, o);      // (a projection keeps the full type tree: its placeholder is the full schema's)
    s->placeholder = std::move(o);
    s->placeholder_done = true;
  }
  return s->placeholder;
}

// ---------------------------------------------------------------------------
// validation
// ---------------------------------------------------------------------------
struct ErrList {
  std::vector<rh::VErr> v;      // ascending by record index
  uint64_t total = 0;           // exact number of malformed records
};

static int call_device(const rh_opts* opts, bool first_of_list) {
  int device = 0;
  if (first_of_list && opts && opts->n_devices > 0 && opts->devices) { HIPCHK(hipSetDevice(opts->devices[0])); return opts->devices[0]; }
  if (opts && opts->device >= 0) { HIPCHK(hipSetDevice(opts->device)); return opts->device; }
  HIPCHK(hipGetDevice(&device));
  return device;
}

// n device-resident records -> appends the malformed ones (index + rec_base) to `out`, at most `cap` of them: all of them
// when there are no more than that, else -- first_on_overflow -- the `cap` lowest, else none.  Returns the exact count.
// `bitmap_out` (optional) receives the lease that holds the bad-record bitmap (one bit per record) at its start.
static uint64_t validate_device_range(rh_schema* s, int device, hipStream_t stream, const uint8_t* d_data, const uint64_t* d_offsets,
                                      uint64_t data_len, uint64_t n, uint64_t rec_base, uint64_t cap, bool first_on_overflow,
                                      std::vector<rh::VErr>& out, Lease* bitmap_out) {
  if (n == 0) return 0;
  if ((uintptr_t)d_data & 15) throw std::invalid_argument("device payload pointer must be 16-byte aligned");
  const CompiledSchema& cs = *s->cs;
  const DeviceProgram& dp = device_program(s, device);
  const uint32_t cap32 = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(cap, n), 0xFFFFFFFFull);
  const uint64_t words = (n + 63) / 64;
  const uint64_t o_list = align_up(8 * words, kAlign);
  const uint64_t o_count = align_up(o_list + sizeof(rh::VErr) * std::max<uint64_t>(cap32, 1), kAlign);
  Lease ws(dev_pool(), o_count + kAlign, device);

  rh::VParams V;
  std::memset(&V, 0, sizeof V);
  V.data = d_data; V.offsets = d_offsets; V.data_len = data_len; V.n = n; V.rec_limit = n;
  V.prog = dp.prog; V.sym_off = dp.sym_off; V.sym_data = dp.sym_data; V.list_depth = cs.list_depth;
  V.bitmap = (uint64_t*)ws.ptr(); V.list = (rh::VErr*)(ws.ptr() + o_list); V.cap = cap32;
  V.count = (unsigned long long*)(ws.ptr() + o_count);
  // the window: the mean tile + 15 % + 2 KiB as the decode kernels size it, two workgroups per CU at least
  const uint32_t fixed = rh_validate_lds_fixed(cs.list_depth);
  const uint64_t lds_cap = 160 * 1024 - 512;
  if (fixed + 4096 + 32 > lds_cap) throw rh::SchemaError("schema needs more LDS than a CDNA4 workgroup has");
  uint64_t win = align_up((data_len / n + 1) * rh::kBlock * 115 / 100 + 2048, 16);
  win = std::max<uint64_t>(win, 8192);
  win = std::min<uint64_t>(win, std::min<uint64_t>((lds_cap - fixed - 32) & ~15ull, fixed + 32 < 80 * 1024 - 8192 ? (80 * 1024 - fixed - 32) & ~15ull : 96 * 1024));
  const long fixed_win = env_long("RUHVRO_HIP_WIN_BYTES", -1, 0, 150 * 1024);
  if (fixed_win >= 0) win = std::min<uint64_t>((uint64_t)fixed_win & ~15ull, (lds_cap - fixed - 32) & ~15ull);
  V.win_bytes = (uint32_t)win;
  const uint32_t lds = fixed + (uint32_t)win + 32;      // + slack: the walk reads 8 bytes at a cursor that may sit at the window's end

  unsigned long long total = 0;
  auto run = [&] {
    HIPCHK(hipMemsetAsync(V.count, 0, 8, stream));
    if (rh_launch_validate(&V, lds, stream)) throw HipError("k_validate launch failed");
    HIPCHK(hipMemcpyAsync(&total, V.count, 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
  };
  run();
  const uint64_t all = total;
  uint64_t listed = all;
  if (all > cap32) {
    listed = 0;
    if (first_on_overflow && cap32 > 0) {
      // the cap32 lowest: the record behind them bounds a second pass that lists nothing at or above it
      std::vector<uint64_t> bm(words);
      HIPCHK(hipMemcpy(bm.data(), V.bitmap, 8 * words, hipMemcpyDeviceToHost));
      uint64_t seen = 0, limit = n;
      for (uint64_t w = 0; w < words && limit == n; w++) {
        const uint64_t c = (uint64_t)__builtin_popcountll(bm[w]);
        if (seen + c <= cap32) { seen += c; continue; }
        uint64_t m = bm[w];
        for (;; m &= m - 1) {
          if (seen == cap32) { limit = w * 64 + (uint64_t)__builtin_ctzll(m); break; }
          seen++;
        }
      }
      V.rec_limit = limit;
      run();
      if (total != cap32) throw std::runtime_error("internal error: two validation passes disagree");
      listed = cap32;
    }
  }
  if (listed) {
    const size_t at = out.size();
    out.resize(at + listed);
    HIPCHK(hipMemcpy(out.data() + at, V.list, sizeof(rh::VErr) * listed, hipMemcpyDeviceToHost));
    std::sort(out.begin() + (long)at, out.end(), [](const rh::VErr& a, const rh::VErr& b) { return a.rec < b.rec; });
    for (size_t i = at; i < out.size(); i++) out[i].rec += rec_base;
  }
  if (bitmap_out) *bitmap_out = std::move(ws);
  return all;
}

// Host records: uploaded in groups (a plain upload, launch, read-back per group), validated by the same kernel.
static void validate_host(rh_schema* s, const Source& src, uint64_t n, const rh_opts* opts, uint64_t cap, bool first_on_overflow, ErrList& el) {
  require_device();
  const int device = call_device(opts, true);
  const uint64_t kGroupRecords = 1u << 20, kGroupBytes = 256ull << 20;
  std::vector<uint64_t> hoff;
  std::vector<uint8_t> hdata;
  for (uint64_t g0 = 0; g0 < n;) {
    uint64_t g1 = g0, bytes = 0;
    while (g1 < n && g1 - g0 < kGroupRecords) {
      const uint64_t len = src.slices() ? src.lens[g1] : src.offsets[g1 + 1] - src.offsets[g1];
      if (g1 > g0 && bytes + len > kGroupBytes) break;
      bytes += len;
      g1++;
    }
    const uint64_t cnt = g1 - g0;
    hoff.resize(cnt + 1);
    const uint8_t* hsrc;
    if (src.slices()) {
      hdata.resize(bytes);
      uint64_t at = 0;
      for (uint64_t i = 0; i < cnt; i++) {
        hoff[i] = at;
        if (src.lens[g0 + i]) std::memcpy(hdata.data() + at, src.ptrs[g0 + i], src.lens[g0 + i]);
        at += src.lens[g0 + i];
      }
      hoff[cnt] = at;
      hsrc = hdata.data();
    } else {
      for (uint64_t i = 0; i <= cnt; i++) hoff[i] = src.offsets[g0 + i] - src.offsets[g0];
      hsrc = src.data + src.offsets[g0];
    }
    Lease d_data(dev_pool(), bytes + 64, device), d_off(dev_pool(), 8 * (cnt + 1), device);
    if (bytes) HIPCHK(hipMemcpy(d_data.ptr(), hsrc, bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_off.ptr(), hoff.data(), 8 * (cnt + 1), hipMemcpyHostToDevice));
    const uint64_t left = el.v.size() < cap ? cap - el.v.size() : 0;
    const uint64_t bad = validate_device_range(s, device, nullptr, d_data.ptr(), (const uint64_t*)d_off.ptr(), bytes, cnt, g0, left,
                                               first_on_overflow, el.v, nullptr);
    el.total += bad;      // (once the list is full a later group lists nothing: the `cap` lowest, or -- !first_on_overflow -- the caller gives up)
    g0 = g1;
  }
}

static std::unique_ptr<rh_record_errors> to_errors(const std::vector<rh::VErr>& v) {
  std::unique_ptr<rh_record_errors> e(new rh_record_errors);
  for (const rh::VErr& x : v) {
    rh::ErrInfo ei; ei.code = x.code; ei.pad = 0; ei.detail = x.detail;
    e->index.push_back(x.rec);
    e->code.push_back((int)x.code);
    e->message.push_back(format_error(ei));
  }
  return e;
}

static void refuse_async(const rh_opts* opts) {
  if (opts && (opts->flags & RH_ASYNC)) throw std::invalid_argument("a tolerant call is synchronous: RH_ASYNC is refused");
}

// ---------------------------------------------------------------------------
// the tolerant calls
// ---------------------------------------------------------------------------
static int decode_host_tolerant(rh_schema* s, const Source& src, uint64_t n, uint64_t num_chunks, const rh_opts* opts, ArrowArray* out_chunks,
                                uint32_t* out_k, rh_stats* stats, uint64_t max_errors, rh_record_errors** errors) {
  refuse_async(opts);
  if (errors) *errors = nullptr;
  count(RH_CTR_TOLERANT_CALLS);
  std::exception_ptr strict;
  try {
    const int rc = decode_host_impl(s, src, n, num_chunks, opts, out_chunks, out_k, stats);
    if (errors) *errors = new rh_record_errors;
    return rc;
  } catch (const RecordDecodeError&) {
    if (max_errors == 0) throw;
    strict = std::current_exception();
  }
  // a producer that is still handing the slices over (rh_opts.ready): the repair needs all of them
  rh_opts o2 = opts ? *opts : default_opts();
  const bool has_handover = opts && opts->struct_size >= offsetof(rh_opts, gathered) + sizeof(uint64_t*);
  if (has_handover && src.slices() && opts->ready) {
    for (uint32_t spins = 0;; spins++) {
      const uint64_t v = __atomic_load_n(opts->ready, __ATOMIC_ACQUIRE);
      if (v == ~0ull) throw std::invalid_argument("the producer of the record slices gave up");
      if (v >= n) break;
      if (spins > 64) std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
  }
  if (has_handover) { o2.ready = nullptr; o2.gathered = nullptr; }
  ErrList el;
  validate_host(s, src, n, opts, max_errors, false, el);
  if (el.total > max_errors) std::rethrow_exception(strict);
  if (el.total == 0) throw std::runtime_error("internal error: the strict decode failed on a record that the validation accepts");
  count(RH_CTR_TOLERANT_REPAIRS);
  const std::vector<uint8_t>& ph = placeholder_datum(s);
  std::vector<const uint8_t*> ptrs(n);
  std::vector<uint64_t> lens(n);
  if (src.slices()) {
    std::copy(src.ptrs, src.ptrs + n, ptrs.begin());
    std::copy(src.lens, src.lens + n, lens.begin());
  } else {
    for (uint64_t i = 0; i < n; i++) { ptrs[i] = src.data + src.offsets[i]; lens[i] = src.offsets[i + 1] - src.offsets[i]; }
  }
  static const uint8_t kNone = 0;
  for (const rh::VErr& e : el.v) { ptrs[e.rec] = ph.empty() ? &kNone : ph.data(); lens[e.rec] = ph.size(); }
  Source patched;
  patched.ptrs = ptrs.data();
  patched.lens = lens.data();
  int rc;
  try {
    rc = decode_host_impl(s, patched, n, num_chunks, &o2, out_chunks, out_k, stats);
  } catch (const RecordDecodeError& e) {
    throw std::runtime_error(std::string("internal error: the repaired input failed to decode: ") + e.what());
  }
  if (has_handover && src.slices() && opts->gathered) __atomic_store_n(opts->gathered, n, __ATOMIC_RELEASE);
  if (errors) *errors = to_errors(el.v).release();
  return rc;
}

static rh_device_result* decode_device_tolerant(rh_schema* s, const uint8_t* d_data, const uint64_t* d_offsets, uint64_t data_len, uint64_t n,
                                                uint64_t num_chunks, const rh_opts* opts, rh_stats* stats, uint64_t max_errors,
                                                rh_record_errors** errors) {
  refuse_async(opts);
  if (errors) *errors = nullptr;
  count(RH_CTR_TOLERANT_CALLS);
  std::exception_ptr strict;
  try {
    rh_device_result* r = decode_device_impl(s, d_data, d_offsets, data_len, n, num_chunks, opts, stats);
    if (errors) *errors = new rh_record_errors;
    return r;
  } catch (const RecordDecodeError&) {
    if (max_errors == 0) throw;
    strict = std::current_exception();
  }
  const int device = call_device(opts, false);
  hipStream_t stream = opts ? (hipStream_t)opts->stream : nullptr;
  ErrList el;
  Lease bitmap;
  el.total = validate_device_range(s, device, stream, d_data, d_offsets, data_len, n, 0, max_errors, false, el.v, &bitmap);
  if (el.total > max_errors) std::rethrow_exception(strict);
  if (el.total == 0) throw std::runtime_error("internal error: the strict decode failed on a record that the validation accepts");
  count(RH_CTR_TOLERANT_REPAIRS);

  // lengths -> offsets -> gather into a new 16-byte aligned payload; the placeholder is read from a small device copy
  const std::vector<uint8_t>& ph = placeholder_datum(s);
  rh::GParams G;
  std::memset(&G, 0, sizeof G);
  G.data = d_data; G.offsets = d_offsets; G.n = n; G.bitmap = (const uint64_t*)bitmap.ptr();
  G.ph_len = (uint32_t)ph.size();
  G.nblocks = (uint32_t)((n + rh::kPatchBlock - 1) / rh::kPatchBlock);
  const uint64_t o_sum = align_up(std::max<uint64_t>(ph.size(), 1), kAlign);
  Lease small(dev_pool(), o_sum + 8ull * G.nblocks, device);
  Lease new_off(dev_pool(), 8 * (n + 1), device);
  if (!ph.empty()) HIPCHK(hipMemcpyAsync(small.ptr(), ph.data(), ph.size(), hipMemcpyHostToDevice, stream));
  G.ph = small.ptr(); G.blocksum = (uint64_t*)(small.ptr() + o_sum); G.new_offsets = (uint64_t*)new_off.ptr();
  if (rh_launch_patch_offsets(&G, stream)) throw HipError("patch (offsets) launch failed");
  uint64_t new_len = 0;
  HIPCHK(hipMemcpyAsync(&new_len, G.new_offsets + n, 8, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  Lease new_data(dev_pool(), new_len + 64, device);
  G.out = new_data.ptr();
  if (rh_launch_patch_gather(&G, stream)) throw HipError("patch (gather) launch failed");
  HIPCHK(hipMemsetAsync(new_data.ptr() + new_len, 0, 64, stream));
  HIPCHK(hipStreamSynchronize(stream));      // (a call that deals its chunk groups to internal streams reads the input from those)
  rh_device_result* r;
  try {
    r = decode_device_impl(s, new_data.ptr(), (const uint64_t*)new_off.ptr(), new_len, n, num_chunks, opts, stats);
  } catch (const RecordDecodeError& e) {
    throw std::runtime_error(std::string("internal error: the repaired input failed to decode: ") + e.what());
  }
  r->patched_data = std::move(new_data);
  r->patched_offsets = std::move(new_off);
  if (errors) *errors = to_errors(el.v).release();
  return r;
}

}  // namespace rhe

// ===========================================================================
// C ABI
// ===========================================================================
// Reader schemas (rh_schema_resolve) are strict-decode only: tolerant resolution is a follow-up
static bool refuse_resolved(const rh_schema* s, char** err) {
  if (!s || !s->cs->resolved) return false;
  if (err) *err = dup_msg("a resolved schema (rh_schema_resolve) takes the strict decode entry points only: validate / decode tolerantly with the writer schema");
  return true;
}

extern "C" {

int rh_schema_placeholder(const rh_schema* s, const uint8_t** bytes, uint64_t* len) {
  if (!s || !bytes || !len || s->cs->resolved) return RH_ERR_ARGUMENT;
  try {
    const std::vector<uint8_t>& ph = placeholder_datum(const_cast<rh_schema*>(s));
    static const uint8_t kNone = 0;
    *bytes = ph.empty() ? &kNone : ph.data();
    *len = ph.size();
    return RH_OK;
  } catch (...) {
    return RH_ERR_SCHEMA;
  }
}

uint64_t rh_record_errors_count(const rh_record_errors* e) { return e ? e->index.size() : 0; }

int rh_record_errors_get(const rh_record_errors* e, uint64_t i, uint64_t* index, int* code, const char** message) {
  if (!e || i >= e->index.size()) return RH_ERR_ARGUMENT;
  if (index) *index = e->index[i];
  if (code) *code = e->code[i];
  if (message) *message = e->message[i].c_str();
  return RH_OK;
}

void rh_record_errors_free(rh_record_errors* e) { delete e; }

static int validate_entry(const rh_schema* s, const Source& src, uint64_t n, const rh_opts* opts, uint64_t max_errors,
                          rh_record_errors** out, uint64_t* total_bad, char** err) {
  if (out) *out = nullptr;
  return guarded(err, [&] {
    ErrList el;
    validate_host(const_cast<rh_schema*>(s), src, n, opts, max_errors, true, el);
    if (total_bad) *total_bad = el.total;
    if (out) *out = to_errors(el.v).release();
    return RH_OK;
  });
}

int rh_validate(const rh_schema* s, const uint8_t* const* ptrs, const uint64_t* lens, uint64_t n, const rh_opts* opts,
                uint64_t max_errors, rh_record_errors** out, uint64_t* total_bad, char** err) {
  if (!s || (n && (!ptrs || !lens))) return RH_ERR_ARGUMENT;
  if (refuse_resolved(s, err)) return RH_ERR_ARGUMENT;
  Source src;
  src.ptrs = ptrs;
  src.lens = lens;
  return validate_entry(s, src, n, opts, max_errors, out, total_bad, err);
}

int rh_validate_packed(const rh_schema* s, const uint8_t* data, const uint64_t* offsets, uint64_t n, const rh_opts* opts,
                       uint64_t max_errors, rh_record_errors** out, uint64_t* total_bad, char** err) {
  if (!s || !offsets) return RH_ERR_ARGUMENT;
  if (refuse_resolved(s, err)) return RH_ERR_ARGUMENT;
  Source src;
  src.data = data;
  src.offsets = offsets;
  return validate_entry(s, src, n, opts, max_errors, out, total_bad, err);
}

int rh_validate_device(const rh_schema* s, const void* d_data, const void* d_offsets, uint64_t data_len, uint64_t n,
                       const rh_opts* opts, uint64_t max_errors, rh_record_errors** out, uint64_t* total_bad, char** err) {
  if (!s) return RH_ERR_ARGUMENT;
  if (out) *out = nullptr;
  if (refuse_resolved(s, err)) return RH_ERR_ARGUMENT;
  return guarded(err, [&] {
    require_device();
    const int device = call_device(opts, false);
    ErrList el;
    el.total = validate_device_range(const_cast<rh_schema*>(s), device, opts ? (hipStream_t)opts->stream : nullptr, (const uint8_t*)d_data,
                                     (const uint64_t*)d_offsets, data_len, n, 0, max_errors, true, el.v, nullptr);
    if (total_bad) *total_bad = el.total;
    if (out) *out = to_errors(el.v).release();
    return RH_OK;
  });
}

int rh_decode_tolerant(const rh_schema* s, const uint8_t* const* ptrs, const uint64_t* lens, uint64_t n, uint64_t num_chunks,
                       const rh_opts* opts, struct ArrowArray* out_chunks, uint32_t* out_k, rh_stats* stats, char** err,
                       uint64_t max_errors, rh_record_errors** errors) {
  if (!s || !out_chunks || (n && (!ptrs || !lens))) return RH_ERR_ARGUMENT;
  if (refuse_resolved(s, err)) return RH_ERR_ARGUMENT;
  return guarded(err, [&] {
    Source src;
    src.ptrs = ptrs;
    src.lens = lens;
    return decode_host_tolerant(const_cast<rh_schema*>(s), src, n, num_chunks, opts, out_chunks, out_k, stats, max_errors, errors);
  });
}

int rh_decode_packed_tolerant(const rh_schema* s, const uint8_t* data, const uint64_t* offsets, uint64_t n, uint64_t num_chunks,
                              const rh_opts* opts, struct ArrowArray* out_chunks, uint32_t* out_k, rh_stats* stats, char** err,
                              uint64_t max_errors, rh_record_errors** errors) {
  if (!s || !offsets || !out_chunks) return RH_ERR_ARGUMENT;
  if (refuse_resolved(s, err)) return RH_ERR_ARGUMENT;
  return guarded(err, [&] {
    Source src;
    src.data = data;
    src.offsets = offsets;
    return decode_host_tolerant(const_cast<rh_schema*>(s), src, n, num_chunks, opts, out_chunks, out_k, stats, max_errors, errors);
  });
}

int rh_decode_device_tolerant(const rh_schema* s, const void* d_data, const void* d_offsets, uint64_t data_len, uint64_t n,
                              uint64_t num_chunks, const rh_opts* opts, rh_device_result** out, rh_stats* stats, char** err,
                              uint64_t max_errors, rh_record_errors** errors) {
  if (!s || !out) return RH_ERR_ARGUMENT;
  if (refuse_resolved(s, err)) return RH_ERR_ARGUMENT;
  return guarded(err, [&] {
    refuse_async(opts);
    require_device();
    Timer t;
    rh_opts pub;
    if (opts) { pub = *opts; pub.flags &= kPublicFlags; }
    *out = decode_device_tolerant(const_cast<rh_schema*>(s), (const uint8_t*)d_data, (const uint64_t*)d_offsets, data_len, n, num_chunks,
                                  opts ? &pub : nullptr, stats, max_errors, errors);
    if (stats) stats->total_ms = t.ms();
    return RH_OK;
  });
}

}  // extern "C"
