// Row filters: the predicate front end (rh_filter_compile), the filter kernel alone (rh_filter_packed /
// rh_filter_device) and the strict decode calls behind it (rh_decode*_where): one careful walk of every record that also
// evaluates the predicate, a compaction of the record list on the device, and the unchanged strict decode of what is left.
// A call that keeps every record decodes its input where it is: no compaction kernel runs and nothing is copied.
#include "engine_internal.h"
#include "filter.h"

extern "C" {
uint32_t rh_filter_lds_fixed(int list_depth);
int rh_launch_filter(const rh::FParams* F, uint32_t lds_bytes, void* stream);
int rh_launch_filter_offsets(const rh::CParams* G, void* stream);
int rh_launch_filter_gather(const rh::CParams* G, void* stream);
}

using namespace rhe;

namespace rhe {

// ---------------------------------------------------------------------------
// the predicate front end
// ---------------------------------------------------------------------------
[[noreturn]] static void where_fail(const std::string& what) { throw rh::SchemaError("where: " + what); }
[[noreturn]] static void field_fail(const std::string& name, const std::string& what) { where_fail("field '" + name + "': " + what); }

static const char* node_kind_name(rh::NodeKind k) {
  switch (k) {
    case rh::NK_RECORD: return "record";
    case rh::NK_UNION: return "union";
    case rh::NK_LIST: return "array";
    case rh::NK_MAP: return "map";
    case rh::NK_BIN: return "fixed / decimal / uuid / duration";
    case rh::NK_NULL: return "null";
    default: return "unsupported";
  }
}

static int parse_cmp(const std::string& name, const char* op) {
  static const char* const kOps[] = {"==", "!=", "<", "<=", ">", ">=", "is_null", "not_null"};
  if (op)
    for (int i = 0; i < 8; i++)
      if (std::strcmp(op, kOps[i]) == 0) return i;
  field_fail(name, std::string("unknown operator '") + (op ? op : "") + "' (one of == != < <= > >= is_null not_null)");
}

static void compile_term(const rh::CompiledSchema& cs, const rh_filter_term& t, uint32_t k, rh::FilterTerm& out, std::vector<uint8_t>& blob) {
  if (!t.name) where_fail("term " + std::to_string(k) + " names no field");
  const std::string name(t.name);
  const rh::AvroType& top = *cs.avro;
  size_t fi = 0;
  while (fi < top.fields.size() && top.fields[fi].name != name) fi++;
  if (fi == top.fields.size()) {
    if (name.find('.') != std::string::npos)
      where_fail("'" + name + "' is a dotted path: only top-level fields of the writer schema can be filtered on");
    where_fail("unknown top-level field '" + name + "' of the writer schema");
  }
  const int cmp = parse_cmp(name, t.op);
  const std::string ops(t.op);
  const int id = cs.nodes[0].children[fi];
  const rh::DecNode& node = cs.nodes[(size_t)id];
  if (node.kind != rh::NK_FIXED && node.kind != rh::NK_STRING && node.kind != rh::NK_ENUM)
    field_fail(name, std::string("a filter on a ") + node_kind_name(node.kind) + " field is not supported yet");
  int pc = -1;
  for (size_t p = 0; p < cs.prog.size(); p++) {
    const rh::Op& o = cs.prog[p];
    if (o.node == id && (o.code == rh::OP_FIXED || o.code == rh::OP_STRING || o.code == rh::OP_ENUM)) { pc = (int)p; break; }
  }
  if (pc < 0 || cs.prog[(size_t)pc].dom != 0) throw std::runtime_error("where: internal error: field '" + name + "' has no leaf op in domain 0");
  const rh::Op& op = cs.prog[(size_t)pc];
  std::memset(&out, 0, sizeof out);
  out.pc = pc;
  out.cmp = (uint32_t)cmp;
  const bool is_int = op.code == rh::OP_FIXED && (op.a == rh::FK_I32 || op.a == rh::FK_I64);
  const bool is_flt = op.code == rh::OP_FIXED && (op.a == rh::FK_F32 || op.a == rh::FK_F64);
  const bool is_bool = op.code == rh::OP_FIXED && op.a == rh::FK_BOOL;
  out.kind = op.code == rh::OP_ENUM ? rh::FLT_ENUM
             : op.code == rh::OP_STRING ? rh::FLT_BYTES
             : op.a == rh::FK_I32 ? rh::FLT_I32
             : op.a == rh::FK_I64 ? rh::FLT_I64
             : op.a == rh::FK_F32 ? rh::FLT_F32
             : op.a == rh::FK_F64 ? rh::FLT_F64 : rh::FLT_BOOL;
  if (cmp == rh::FC_IS_NULL || cmp == rh::FC_NOT_NULL) {
    if (t.value_kind != RH_FILTER_VALUE_NONE) field_fail(name, "operator '" + ops + "' takes no value");
    return;
  }
  if (t.value_kind == RH_FILTER_VALUE_NONE)
    field_fail(name, "operator '" + ops + "' needs a value (a null matches no comparison: use is_null / not_null)");
  const bool ordered = cmp != rh::FC_EQ && cmp != rh::FC_NE;
  if (is_int) {
    if (t.value_kind == RH_FILTER_VALUE_BOOL) field_fail(name, "an int / long field compares with an int, not with a bool");
    if (t.value_kind == RH_FILTER_VALUE_BIGINT) field_fail(name, "the value is outside the int64 range");
    if (t.value_kind != RH_FILTER_VALUE_INT) field_fail(name, "an int / long field compares with an int");
    out.i = t.i;
  } else if (is_flt) {
    if (t.value_kind != RH_FILTER_VALUE_INT && t.value_kind != RH_FILTER_VALUE_DOUBLE && t.value_kind != RH_FILTER_VALUE_BIGINT)
      field_fail(name, "a float / double field compares with a float or an int");
    out.d = t.d;
  } else if (is_bool) {
    if (ordered) field_fail(name, "operator '" + ops + "' does not apply to a boolean field (== and != only)");
    if (t.value_kind != RH_FILTER_VALUE_BOOL) field_fail(name, "a boolean field compares with a bool");
    out.i = t.i ? 1 : 0;
  } else if (op.code == rh::OP_STRING) {
    if (t.value_kind != RH_FILTER_VALUE_BYTES) field_fail(name, "a string / bytes field compares with a str or bytes");
    if (t.len > rh::kMaxFilterBytes)
      field_fail(name, "the value has " + std::to_string(t.len) + " bytes: a comparand of more than " + std::to_string(rh::kMaxFilterBytes) + " bytes is not supported");
    if (t.len && !t.bytes) field_fail(name, "the value has no bytes");
    out.boff = (uint32_t)blob.size();
    out.blen = (uint32_t)t.len;
    blob.insert(blob.end(), t.bytes, t.bytes + t.len);
  } else {      // enum
    if (ordered) field_fail(name, "operator '" + ops + "' does not apply to an enum field (== and != only)");
    if (t.value_kind != RH_FILTER_VALUE_BYTES) field_fail(name, "an enum field compares with a symbol name (a str)");
    const std::string sym(t.len ? (const char*)t.bytes : "", (size_t)t.len);
    int found = -1;
    for (int s = 0; s < op.c && found < 0; s++) {
      const uint32_t a = cs.sym_off[(size_t)(op.b + s)], b = cs.sym_off[(size_t)(op.b + s + 1)];
      if (b - a == sym.size() && std::memcmp(cs.sym_data.data() + a, sym.data(), sym.size()) == 0) found = s;
    }
    if (found < 0) field_fail(name, "'" + sym + "' is not a symbol of the enum");
    out.i = found;
  }
}

static std::unique_ptr<rh_filter> compile_filter(const rh_schema* writer, const rh_filter_term* terms, uint32_t n) {
  if (writer->cs->projected || writer->cs->resolved)
    throw std::invalid_argument("where: the predicate compiles against the plain writer schema (not a projection or a resolution)");
  if (n == 0) where_fail("the predicate has no terms (pass None for no filter)");
  if (n > rh::kMaxFilterTerms) where_fail("the predicate has " + std::to_string(n) + " terms: more than " + std::to_string(rh::kMaxFilterTerms) + " are not supported");
  if (!terms) throw std::invalid_argument("where: null term list");
  std::unique_ptr<rh_filter> f(new rh_filter);
  std::memset(&f->prog, 0, sizeof f->prog);
  f->prog.nterms = n;
  for (uint32_t k = 0; k < n; k++) compile_term(*writer->cs, terms[k], k, f->prog.term[k], f->bytes);
  f->json = writer->cs->json;
  return f;
}

// ---------------------------------------------------------------------------
// the filter on n device-resident records
// ---------------------------------------------------------------------------
static std::mutex g_last_mu;
static float g_last_filter_ms = 0, g_last_gather_ms = 0;
static uint64_t g_last_n = 0, g_last_kept = 0;
static void note_last(float filter_ms, float gather_ms, uint64_t n, uint64_t kept) {
  std::lock_guard<std::mutex> g(g_last_mu);
  g_last_filter_ms = filter_ms; g_last_gather_ms = gather_ms; g_last_n = n; g_last_kept = kept;
}

static void refuse_opts(const rh_opts* opts) {
  if (opts && opts->n_devices > 0) throw std::invalid_argument("where: a filtered call runs on one device (rh_opts.devices is refused)");
  if (opts && (opts->flags & RH_ASYNC)) throw std::invalid_argument("where: a filtered call is synchronous: RH_ASYNC is refused");
}

static int call_device(const rh_opts* opts) {
  int device = 0;
  if (opts && opts->device >= 0) { HIPCHK(hipSetDevice(opts->device)); return opts->device; }
  HIPCHK(hipGetDevice(&device));
  return device;
}

struct Filtered {
  Lease ws;                 // the keep bitmap at its start (one bit per record)
  uint64_t kept = 0;
  float filter_ms = 0;
};

// Runs rh_k_filter; throws the strict decode's error for the lowest malformed record.
static void filter_device_range(rh_filter* f, int device, hipStream_t stream, const uint8_t* d_data, const uint64_t* d_offsets, uint64_t data_len,
                                uint64_t n, Filtered& out) {
  out.kept = 0;
  out.filter_ms = 0;
  if (n == 0) return;
  if ((uintptr_t)d_data & 15) throw std::invalid_argument("device payload pointer must be 16-byte aligned");
  rh_schema* s = f->plain;
  const CompiledSchema& cs = *s->cs;
  const DeviceProgram& dp = device_program(s, device);
  const uint32_t cap = 64;
  const uint64_t words = rh::filter_words(n);
  const uint64_t o_bad = align_up(8 * words, kAlign);
  const uint64_t o_list = align_up(o_bad + 8 * words, kAlign);
  const uint64_t o_count = align_up(o_list + sizeof(rh::VErr) * cap, kAlign);      // count, then the kept slots
  const uint64_t o_bytes = align_up(o_count + 8 + 8 * rh::kFilterSlots, kAlign);
  Lease ws(dev_pool(), o_bytes + align_up(std::max<uint64_t>(f->bytes.size(), 1), kAlign), device);

  rh::FParams F;
  std::memset(&F, 0, sizeof F);
  F.data = d_data; F.offsets = d_offsets; F.data_len = data_len; F.n = n; F.rec_limit = n;
  F.prog = dp.prog; F.sym_off = dp.sym_off; F.sym_data = dp.sym_data; F.list_depth = cs.list_depth;
  F.keep = (uint64_t*)ws.ptr(); F.bad = (uint64_t*)(ws.ptr() + o_bad); F.list = (rh::VErr*)(ws.ptr() + o_list); F.cap = cap;
  F.count = (unsigned long long*)(ws.ptr() + o_count); F.kept = F.count + 1;
  F.cbytes = ws.ptr() + o_bytes;
  F.flt = f->prog;
  // the window: sized as the validation kernel's (engine_tolerant.cpp), two workgroups per CU at least
  const uint32_t fixed = rh_filter_lds_fixed(cs.list_depth);
  const uint64_t lds_cap = 160 * 1024 - 512;
  if (fixed + 4096 + 32 > lds_cap) throw rh::SchemaError("schema needs more LDS than a CDNA4 workgroup has");
  uint64_t win = align_up((data_len / n + 1) * rh::kBlock * 115 / 100 + 2048, 16);
  win = std::max<uint64_t>(win, 8192);
  win = std::min<uint64_t>(win, std::min<uint64_t>((lds_cap - fixed - 32) & ~15ull, fixed + 32 < 80 * 1024 - 8192 ? (80 * 1024 - fixed - 32) & ~15ull : 96 * 1024));
  const long fixed_win = env_long("RUHVRO_HIP_WIN_BYTES", -1, 0, 150 * 1024);
  if (fixed_win >= 0) win = std::min<uint64_t>((uint64_t)fixed_win & ~15ull, (lds_cap - fixed - 32) & ~15ull);
  F.win_bytes = (uint32_t)win;
  const uint32_t lds = fixed + (uint32_t)win + 32;      // + slack: the walk reads 8 bytes at a cursor that may sit at the window's end

  if (!f->bytes.empty()) HIPCHK(hipMemcpyAsync(ws.ptr() + o_bytes, f->bytes.data(), f->bytes.size(), hipMemcpyHostToDevice, stream));
  Events ev;
  ev.init();
  unsigned long long head[1 + rh::kFilterSlots];
  auto run = [&] {
    HIPCHK(hipMemsetAsync(F.count, 0, 8 + 8 * rh::kFilterSlots, stream));
    ev.rec(0, stream);
    if (rh_launch_filter(&F, lds, stream)) throw HipError("k_filter launch failed");
    ev.rec(1, stream);
    HIPCHK(hipMemcpyAsync(head, F.count, sizeof head, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
  };
  run();
  out.filter_ms = ev.ms(0, 1);
  if (head[0]) {
    // the lowest malformed record: in the list when all of them are, else found in the bitmap and listed alone by a second pass
    rh::VErr lowest;
    if (head[0] <= cap) {
      std::vector<rh::VErr> v((size_t)head[0]);
      HIPCHK(hipMemcpy(v.data(), F.list, sizeof(rh::VErr) * v.size(), hipMemcpyDeviceToHost));
      lowest = *std::min_element(v.begin(), v.end(), [](const rh::VErr& a, const rh::VErr& b) { return a.rec < b.rec; });
    } else {
      std::vector<uint64_t> bm(words);
      HIPCHK(hipMemcpy(bm.data(), F.bad, 8 * words, hipMemcpyDeviceToHost));
      uint64_t lo = n;
      for (uint64_t w = 0; w < words && lo == n; w++)
        if (bm[w]) lo = w * 64 + (uint64_t)__builtin_ctzll(bm[w]);
      F.rec_limit = lo + 1;
      run();
      if (head[0] != 1) throw std::runtime_error("internal error: two filter passes disagree");
      HIPCHK(hipMemcpy(&lowest, F.list, sizeof lowest, hipMemcpyDeviceToHost));
    }
    rh::ErrInfo ei; ei.code = lowest.code; ei.pad = 0; ei.detail = lowest.detail;
    throw RecordDecodeError(format_error(ei));
  }
  for (uint32_t i = 0; i < rh::kFilterSlots; i++) out.kept += head[1 + i];
  if (out.kept > n) throw std::runtime_error("internal error: the filter kept more records than it was given");
  out.ws = std::move(ws);
}

void check_filter(const rh_schema* s, const rh_filter* f) {
  if (s->cs->json != f->json) throw std::invalid_argument("where: the predicate was compiled against another writer schema");
}

void compact_kept(const uint8_t* d_data, const uint64_t* d_offsets, uint64_t data_len, uint64_t n, const uint64_t* d_keep, uint64_t kept,
                  int device, hipStream_t stream, Compacted& out) {
  rh::CParams G;
  std::memset(&G, 0, sizeof G);
  G.data = d_data; G.offsets = d_offsets; G.n = n; G.keep = d_keep;
  G.nblocks = (uint32_t)((n + rh::kFilterBlock - 1) / rh::kFilterBlock);
  const uint64_t o_bytes = align_up(8ull * G.nblocks, kAlign);
  const uint64_t o_rank = align_up(o_bytes + 8ull * G.nblocks, kAlign);
  Lease small(dev_pool(), o_rank + 8 * rh::filter_words(n), device);
  Lease new_off(dev_pool(), 8 * (kept + 1), device);
  G.blockcnt = (uint64_t*)small.ptr(); G.blockbytes = (uint64_t*)(small.ptr() + o_bytes); G.wordrank = (uint64_t*)(small.ptr() + o_rank);
  G.new_offsets = (uint64_t*)new_off.ptr();
  Events ev;
  ev.init();
  ev.rec(0, stream);
  if (rh_launch_filter_offsets(&G, stream)) throw HipError("filter (offsets) launch failed");
  uint64_t new_len = 0;
  HIPCHK(hipMemcpyAsync(&new_len, G.new_offsets + kept, 8, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  if (new_len > data_len) throw std::runtime_error("internal error: the kept records are larger than the input");
  Lease new_data(dev_pool(), new_len + 64, device);
  G.out = new_data.ptr();
  if (rh_launch_filter_gather(&G, stream)) throw HipError("filter (gather) launch failed");
  ev.rec(1, stream);
  HIPCHK(hipMemsetAsync(new_data.ptr() + new_len, 0, 64, stream));
  HIPCHK(hipStreamSynchronize(stream));      // (a call that deals its chunk groups to internal streams reads the input from those)
  out.ms = ev.ms(0, 1);
  out.len = new_len;
  out.data = std::move(new_data);
  out.off = std::move(new_off);
}

// filter -> (errors) -> kept == n: the input as it is | compact -> the strict decode of the compacted list
static rh_device_result* decode_device_where(rh_schema* s, rh_filter* f, const uint8_t* d_data, const uint64_t* d_offsets, uint64_t data_len,
                                             uint64_t n, uint64_t num_chunks, const rh_opts* opts, rh_stats* stats, uint64_t* kept_out) {
  refuse_opts(opts);
  check_filter(s, f);
  const int device = call_device(opts);
  hipStream_t stream = opts ? (hipStream_t)opts->stream : nullptr;
  Filtered fl;
  filter_device_range(f, device, stream, d_data, d_offsets, data_len, n, fl);
  if (kept_out) *kept_out = fl.kept;
  if (fl.kept == n) {
    note_last(fl.filter_ms, 0, n, fl.kept);
    fl.ws.release();
    return decode_device_impl(s, d_data, d_offsets, data_len, n, num_chunks, opts, stats);
  }
  Compacted c;
  compact_kept(d_data, d_offsets, data_len, n, (const uint64_t*)fl.ws.ptr(), fl.kept, device, stream, c);
  note_last(fl.filter_ms, c.ms, n, fl.kept);
  fl.ws.release();
  rh_device_result* r;
  try {
    r = decode_device_impl(s, c.data.ptr(), (const uint64_t*)c.off.ptr(), c.len, fl.kept, num_chunks, opts, stats);
  } catch (const RecordDecodeError& e) {
    throw std::runtime_error(std::string("internal error: a record the filter accepted failed to decode: ") + e.what());
  }
  r->patched_data = std::move(c.data);      // the result owns every byte its call read (as a repaired tolerant call's)
  r->patched_offsets = std::move(c.off);
  return r;
}

// host records -> one plain upload (not the pinned, pipelined list path of rh_decode); also the framed calls' (engine_frame.cpp)
void upload(const Source& src, uint64_t n, int device, hipStream_t stream, Uploaded& u) {
  std::vector<uint64_t> hoff(n + 1);
  std::vector<uint8_t> hdata;
  const uint8_t* hsrc = nullptr;
  if (src.slices()) {
    uint64_t at = 0;
    for (uint64_t i = 0; i < n; i++) { hoff[i] = at; at += src.lens[i]; }
    hoff[n] = at;
    hdata.resize(at);
    for (uint64_t i = 0; i < n; i++)
      if (src.lens[i]) std::memcpy(hdata.data() + hoff[i], src.ptrs[i], src.lens[i]);
    hsrc = hdata.data();
    u.bytes = at;
  } else {
    const uint64_t base = n ? src.offsets[0] : 0;
    for (uint64_t i = 0; i <= n; i++) {
      if (i && src.offsets[i] < src.offsets[i - 1]) throw std::invalid_argument("record offsets must not decrease");
      hoff[i] = (n ? src.offsets[i] : 0) - base;
    }
    hsrc = src.data + base;
    u.bytes = hoff[n];
  }
  u.data = Lease(dev_pool(), u.bytes + 64, device);
  u.off = Lease(dev_pool(), 8 * (n + 1), device);
  if (u.bytes) HIPCHK(hipMemcpyAsync(u.data.ptr(), hsrc, u.bytes, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemsetAsync(u.data.ptr() + u.bytes, 0, 64, stream));
  HIPCHK(hipMemcpyAsync(u.off.ptr(), hoff.data(), 8 * (n + 1), hipMemcpyHostToDevice, stream));
  HIPCHK(hipStreamSynchronize(stream));
}

static int decode_host_where(const rh_schema* s, const rh_filter* f, const Source& src, uint64_t n, uint64_t num_chunks, const rh_opts* opts,
                             ArrowArray* out_chunks, uint32_t* out_k, rh_stats* stats, uint64_t* kept) {
  refuse_opts(opts);
  require_device();
  Timer t;
  rh_opts pub;
  if (opts) { pub = *opts; pub.flags &= kPublicFlags; }
  const int device = call_device(opts);
  hipStream_t stream = opts ? (hipStream_t)opts->stream : nullptr;
  Uploaded u;
  Timer tu;
  upload(src, n, device, stream, u);
  const float up_ms = tu.ms();
  std::unique_ptr<rh_device_result> r(decode_device_where(const_cast<rh_schema*>(s), const_cast<rh_filter*>(f), u.data.ptr(),
                                                          (const uint64_t*)u.off.ptr(), u.bytes, n, num_chunks, opts ? &pub : nullptr, stats, kept));
  if (stats) stats->h2d_ms += up_ms;
  Timer td;
  const int rc = to_host_impl(r.get(), out_chunks, stream);
  if (stats) stats->d2h_ms = td.ms();
  if (out_k) *out_k = r->k;
  if (stats) stats->total_ms = t.ms();
  return rc;
}

static int filter_host(const rh_filter* f, const Source& src, uint64_t n, const rh_opts* opts, uint64_t* keep_words, uint64_t* kept) {
  refuse_opts(opts);
  require_device();
  const int device = call_device(opts);
  hipStream_t stream = opts ? (hipStream_t)opts->stream : nullptr;
  Uploaded u;
  upload(src, n, device, stream, u);
  Filtered fl;
  filter_device_range(const_cast<rh_filter*>(f), device, stream, u.data.ptr(), (const uint64_t*)u.off.ptr(), u.bytes, n, fl);
  if (n && keep_words) HIPCHK(hipMemcpy(keep_words, fl.ws.ptr(), 8 * rh::filter_words(n), hipMemcpyDeviceToHost));
  if (kept) *kept = fl.kept;
  note_last(fl.filter_ms, 0, n, fl.kept);
  return RH_OK;
}

}  // namespace rhe

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

int rh_filter_compile(const rh_schema* writer, const rh_filter_term* terms, uint32_t n, rh_filter** out, char** err) {
  if (!writer || !out) return RH_ERR_ARGUMENT;
  *out = nullptr;
  return guarded(err, [&] {
    std::unique_ptr<rh_filter> f = compile_filter(writer, terms, n);
    char* e2 = nullptr;
    f->plain = rh_schema_compile(f->json.data(), f->json.size(), &e2);
    if (!f->plain) {
      const std::string m = e2 ? e2 : "schema compile failed";
      rh_free_string(e2);
      throw rh::SchemaError(m);
    }
    *out = f.release();
    return RH_OK;
  });
}

void rh_filter_free(rh_filter* f) {
  if (!f) return;
  rh_schema_free(f->plain);
  delete f;
}

int rh_filter_packed(const rh_filter* f, const uint8_t* data, const uint64_t* offsets, uint64_t n, const rh_opts* opts,
                     uint64_t* keep_words, uint64_t* kept, char** err) {
  if (!f || !offsets) return RH_ERR_ARGUMENT;
  return guarded(err, [&] {
    Source src;
    src.data = data;
    src.offsets = offsets;
    return filter_host(f, src, n, opts, keep_words, kept);
  });
}

int rh_filter_device(const rh_filter* f, const void* d_data, const void* d_offsets, uint64_t data_len, uint64_t n, const rh_opts* opts,
                     uint64_t* keep_words, uint64_t* kept, char** err) {
  if (!f) return RH_ERR_ARGUMENT;
  return guarded(err, [&] {
    refuse_opts(opts);
    require_device();
    const int device = call_device(opts);
    Filtered fl;
    filter_device_range(const_cast<rh_filter*>(f), device, opts ? (hipStream_t)opts->stream : nullptr, (const uint8_t*)d_data,
                        (const uint64_t*)d_offsets, data_len, n, fl);
    if (n && keep_words) HIPCHK(hipMemcpy(keep_words, fl.ws.ptr(), 8 * rh::filter_words(n), hipMemcpyDeviceToHost));
    if (kept) *kept = fl.kept;
    note_last(fl.filter_ms, 0, n, fl.kept);
    return RH_OK;
  });
}

int rh_decode_where(const rh_schema* s, const uint8_t* const* ptrs, const uint64_t* lens, uint64_t n, uint64_t num_chunks,
                    const rh_opts* opts, struct ArrowArray* out_chunks, uint32_t* out_k, rh_stats* stats, char** err,
                    const rh_filter* filter, uint64_t* kept) {
  if (!s || !filter || !out_chunks || (n && (!ptrs || !lens))) return RH_ERR_ARGUMENT;
  return guarded(err, [&] {
    Source src;
    src.ptrs = ptrs;
    src.lens = lens;
    return decode_host_where(s, filter, src, n, num_chunks, opts, out_chunks, out_k, stats, kept);
  });
}

int rh_decode_packed_where(const rh_schema* s, const uint8_t* data, const uint64_t* offsets, uint64_t n, uint64_t num_chunks,
                           const rh_opts* opts, struct ArrowArray* out_chunks, uint32_t* out_k, rh_stats* stats, char** err,
                           const rh_filter* filter, uint64_t* kept) {
  if (!s || !filter || !offsets || !out_chunks) return RH_ERR_ARGUMENT;
  return guarded(err, [&] {
    Source src;
    src.data = data;
    src.offsets = offsets;
    return decode_host_where(s, filter, src, n, num_chunks, opts, out_chunks, out_k, stats, kept);
  });
}

int rh_decode_device_where(const rh_schema* s, const void* d_data, const void* d_offsets, uint64_t data_len, uint64_t n,
                           uint64_t num_chunks, const rh_opts* opts, rh_device_result** out, rh_stats* stats, char** err,
                           const rh_filter* filter, uint64_t* kept) {
  if (!s || !filter || !out) return RH_ERR_ARGUMENT;
  *out = nullptr;
  return guarded(err, [&] {
    refuse_opts(opts);
    require_device();
    Timer t;
    rh_opts pub;
    if (opts) { pub = *opts; pub.flags &= kPublicFlags; }
    *out = decode_device_where(const_cast<rh_schema*>(s), const_cast<rh_filter*>(filter), (const uint8_t*)d_data, (const uint64_t*)d_offsets,
                               data_len, n, num_chunks, opts ? &pub : nullptr, stats, kept);
    if (stats) stats->total_ms = t.ms();
    return RH_OK;
  });
}

void rh_filter_last(float* filter_ms, float* gather_ms, uint64_t* n, uint64_t* kept) {
  std::lock_guard<std::mutex> g(g_last_mu);
  if (filter_ms) *filter_ms = g_last_filter_ms;
  if (gather_ms) *gather_ms = g_last_gather_ms;
  if (n) *n = g_last_n;
  if (kept) *kept = g_last_kept;
}

}  // extern "C"
