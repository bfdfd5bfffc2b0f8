// Per-schema kernel specialisation: compiled schema -> HIP source -> gfx950 code object.
//
// The schema program (program.h) that the generic interpreter fetches op by op is
// emitted here as a straight-line call sequence over the SAME field handlers
// (walk.h) with constexpr Ops, wrapped by the kernel bodies of spec_body.h.
// hiprtc compiles it for gfx950 (no GPU needed to compile); code objects are cached
// on disk by content hash, next to the library (pre-populated by build() for the
// benchmark schemas) so a process normally only loads them.
//
// The reference caches one parsed schema per schema string for the life of the
// process (src/lib.rs:35-54); the specialised kernel is the same idea one level
// down: one decoder per schema, built once.
#include "specialize.h"

#include <dlfcn.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <mutex>
#include <sstream>

#include "rtc_compile.h"
#include "walk_resolve.h"

namespace rh {

namespace {

const char* op_name(int code) {
  switch (code) {
    case OP_FIXED: return "OP_FIXED";
    case OP_STRING: return "OP_STRING";
    case OP_ENUM: return "OP_ENUM";
    case OP_REC_BEGIN: return "OP_REC_BEGIN";
    case OP_REC_END: return "OP_REC_END";
    case OP_UNION_BEGIN: return "OP_UNION_BEGIN";
    case OP_VARIANT: return "OP_VARIANT";
    case OP_BIN: return "OP_BIN";
    case OP_UNION_END: return "OP_UNION_END";
    case OP_LIST_BEGIN: return "OP_LIST_BEGIN";
    case OP_LIST_NEXT: return "OP_LIST_NEXT";
    case OP_LIST_TAIL: return "OP_LIST_TAIL";
    case OP_LIST_END: return "OP_LIST_END";
    default: return "OP_END";
  }
}

}  // namespace

// records per tile of a schema's specialised kernels: one wavefront for a wide schema (program.h kWideTile), else the default
int spec_tile_records(const CompiledSchema& cs) { return cs.wide ? kWideTile : spec_tile_records(); }

int spec_tile_records() {
  static const int v = [] {
    const char* e = std::getenv("RUHVRO_HIP_TILE");
    const int t = e ? std::atoi(e) : 256;
    return (t == 64 || t == 128 || t == 256 || t == 512 || t == 1024) ? t : 256;      // (wavefronts per workgroup: a power of two)
  }();
  return v;
}

// RUHVRO_HIP_VARIANT=NAME[,NAME...] -> "#define RH_V_NAME 1" lines in front of the generated source: experimental
// code paths of the device headers that are staged for an A/B on the GPU (`#ifdef RH_V_NAME`; each has its own
// kernel-cache entry, since the key hashes the source).  Unset = the validated default kernels, byte for byte.
// A variant that wins is made the default and its #ifdef removed; one that loses is deleted (scripts/gpu_ab.sh).
// (generate_lean_source: LEN16 and INT28 count as named, whatever the variable says)
static thread_local bool t_lean = false;

static void emit_variant_defines(std::ostringstream& o) {
  const char* e = std::getenv("RUHVRO_HIP_VARIANT");
  std::vector<std::string> names;
  std::string name;
  for (const char* p = e ? e : "";; p++) {
    if (*p == ',' || *p == 0) {
      bool ok = !name.empty();
      for (char ch : name) ok = ok && ((ch >= 'A' && ch <= 'Z') || (ch >= '0' && ch <= '9') || ch == '_');
      if (ok) names.push_back(name);
      name.clear();
      if (*p == 0) break;
    } else {
      name.push_back(*p);
    }
  }
  if (t_lean)
    for (const char* n : {"LEN16", "INT28"})
      if (std::find(names.begin(), names.end(), n) == names.end()) names.push_back(n);
  for (const std::string& n : names) o << "#define RH_V_" << n << " 1\n";
}

static bool variant_on(const char* name) {
  if (t_lean && (!std::strcmp(name, "LEN16") || !std::strcmp(name, "INT28"))) return true;
  const char* e = std::getenv("RUHVRO_HIP_VARIANT");
  if (!e) return false;
  const std::string all = std::string(",") + e + ",";
  return all.find(std::string(",") + name + ",") != std::string::npos;
}

// Top-level arrays / maps without nested lists: pc of LIST_BEGIN -> index among the schema's dense lists.
static std::map<size_t, int> dense_lists(const CompiledSchema& cs) {
  std::map<size_t, int> out;
  static const bool off = [] { const char* e = std::getenv("RUHVRO_HIP_NO_DENSE"); return e && *e && *e != '0'; }();
  if (off) return out;
  for (size_t i = 0; i < cs.prog.size(); i++) {
    const Op& p = cs.prog[i];
    if (p.code == OP_END) break;
    if (p.code != OP_LIST_BEGIN || p.dom != 0 || p.c != 0 || (p.flags & F_DROP)) continue;      // (a dropped list is an ordinary skipped loop)
    bool leaf = true;
    size_t j = i + 1;
    for (; j < cs.prog.size() && cs.prog[j].code != OP_LIST_END; j++)
      if (cs.prog[j].code == OP_LIST_BEGIN) { leaf = false; break; }
    if (leaf && j < cs.prog.size() && cs.prog[i + 1].code == OP_LIST_NEXT) {
      const int id = (int)out.size();
      out[i] = id;
    }
  }
  return out;
}

int dense_list_count(const CompiledSchema& cs) { return (int)dense_lists(cs).size(); }

std::string generate_kernel_source(const CompiledSchema& cs, unsigned parts) {
  std::ostringstream o;
  o << "// generated by ruhvro_hip specialize.cpp -- do not edit\n";
  emit_variant_defines(o);
  if (const char* e = std::getenv("RUHVRO_HIP_PROFILE"))
    if (*e && *e != '0') o << "#define RH_PROFILE 1\n";
  if (cs.wide) o << "#define RH_WIDE_SCHEMA 1\n";
  if (cs.max_nest > kShallowNest || cs.max_union_depth > kShallowUnionDepth) o << "#define RH_DEEP 1\n";      // (walk.h: 64 / 128-bit stacks)
  o << "#include \"spec_body.h\"\n";
  if (cs.projected) o << "#include \"walk_drop.h\"\n";      // (projection: the ops of dropped fields, DropCtx)
  if (cs.resolved) o << "#include \"walk_resolve.h\"\n";      // (reader schema: promoted and defaulted leaves)
  // a schema whose calls have no size pass: its emit kernels walk and count the tiles past the LDS window themselves (spec_flat.h)
  const bool flat = cs.K == 0 && !cs.size_always;
  if (flat) o << "#include \"spec_flat.h\"\n";
  o << "namespace rh {\n";
  o << "struct Spec {\n";
  o << "  static constexpr int TILE = " << spec_tile_records(cs) << ";   // records (= threads) per workgroup\n";
  o << "  static constexpr int K = " << cs.K << ", KL = " << cs.KL << ", NDOM = " << cs.ndom << ", NBUF = " << cs.bufs.size()
    << ", NNODES = " << cs.nodes.size() << ", DEPTH = " << cs.list_depth << ";\n";
  o << "  static constexpr int databuf(int k) {\n    switch (k) {\n";
  for (size_t b = 0; b < cs.bufs.size(); b++)
    if (cs.bufs[b].kind == BK_DATA) o << "      case " << cs.bufs[b].counter << ": return " << b << ";\n";
  o << "      default: return 0;\n    }\n  }\n";
  {   // child-domain bitmaps built in LDS (spec_body.h SCtx::set_bit): slot <-> (buffer id, row domain)
    std::vector<int> bm;
    for (size_t b = 0; b < cs.bufs.size(); b++)
      if (cs.bufs[b].kind == BK_BITMAP && cs.bufs[b].dom != 0) bm.push_back((int)b);
    o << "  static constexpr int NBM = " << bm.size() << ";\n";
    o << "  static constexpr int bmslot(int buf) {\n    switch (buf) {\n";
    for (size_t i = 0; i < bm.size(); i++) o << "      case " << bm[i] << ": return " << i << ";\n";
    o << "      default: return 0;\n    }\n  }\n";
    o << "  static constexpr int bmbuf(int slot) {\n    switch (slot) {\n";
    for (size_t i = 0; i < bm.size(); i++) o << "      case " << i << ": return " << bm[i] << ";\n";
    o << "      default: return 0;\n    }\n  }\n";
    o << "  static constexpr int bmdom(int slot) {\n    switch (slot) {\n";
    for (size_t i = 0; i < bm.size(); i++) o << "      case " << i << ": return " << cs.bufs[bm[i]].dom << ";\n";
    o << "      default: return 1;\n    }\n  }\n";
  }
  {   // domain-0 bitmaps (validity / boolean values of rows that line up with lanes): slot <-> buffer id (SCtx::put_word0)
    std::vector<int> b0;
    for (size_t b = 0; b < cs.bufs.size(); b++)
      if (cs.bufs[b].kind == BK_BITMAP && cs.bufs[b].dom == 0) b0.push_back((int)b);
    o << "  static constexpr int NB0 = " << b0.size() << ";\n";
    o << "  static constexpr int bm0slot(int buf) {\n    switch (buf) {\n";
    for (size_t i = 0; i < b0.size(); i++) o << "      case " << b0[i] << ": return " << i << ";\n";
    o << "      default: return 0;\n    }\n  }\n";
    o << "  static constexpr int bm0buf(int slot) {\n    switch (slot) {\n";
    for (size_t i = 0; i < b0.size(); i++) o << "      case " << i << ": return " << b0[i] << ";\n";
    o << "      default: return 0;\n    }\n  }\n";
  }
  // item-dense lists (spec_body.h dense_list): the string counters their bodies advance
  const std::map<size_t, int> dense = dense_lists(cs);
  o << "  static constexpr int NDENSE = " << dense.size() << ";\n";
  o << "  static constexpr bool dense_body(int list, int k) {\n    switch (list) {\n";
  for (const auto& kv : dense) {
    o << "      case " << kv.second << ": return false";
    for (size_t j = kv.first + 1; cs.prog[j].code != OP_LIST_END; j++)
      if (cs.prog[j].code == OP_STRING || cs.prog[j].code == OP_ENUM) o << " || k == " << cs.prog[j].a;
    o << ";\n";
  }
  o << "      default: return false;\n    }\n  }\n";
  // ... and, for a list whose body is ONE plain string (array<string>: what a giant record usually is made of), that string's
  // counter: item_scan decodes such candidates by hand instead of through the handler (spec_body.h)
  o << "  static constexpr int dense_str(int list) {\n    switch (list) {\n";
  for (const auto& kv : dense) {
    const size_t b = kv.first + 2;
    if (b + 1 < cs.prog.size() && cs.prog[b].code == OP_STRING && !(cs.prog[b].flags & F_NULLABLE) && cs.prog[b + 1].code == OP_LIST_TAIL)
      o << "      case " << kv.second << ": return " << cs.prog[b].a << ";\n";
  }
  o << "      default: return -1;\n    }\n  }\n";
  // Enum symbols as immediates (walk.h h_string): an enum of few, short symbols gets its (length, bytes) by a compare /
  // select chain on the index instead of two dependent trips to global memory (sym_off, then sym_data) per field.
  // Used by the size pass, which needs the length.  RUHVRO_HIP_NO_ENUM_IMM=1: A/B knob.
  o << "  static __device__ __forceinline__ bool enum_sym(int b, uint32_t v, uint32_t& len, uint64_t& bits) {\n";
  if (!std::getenv("RUHVRO_HIP_NO_ENUM_IMM")) {
    std::map<int, int> seen;        // first symbol index -> symbol count
    for (const Op& p : cs.prog)
      if (p.code == OP_ENUM && !(p.flags & F_DROP)) seen[p.b] = p.c;      // (a dropped enum needs its index checked, not its text)
    for (const auto& kv : seen) {
      const int b = kv.first, ns = kv.second;
      bool small = ns >= 1 && ns <= 16;
      for (int i = 0; small && i < ns; i++) small = cs.sym_off[(size_t)b + i + 1] - cs.sym_off[(size_t)b + i] <= 8;
      if (!small) continue;
      std::ostringstream ls, bs;
      uint32_t longest = 0;
      bool same_len = true;
      for (int i = 0; i < ns; i++) {
        const uint32_t l = cs.sym_off[(size_t)b + i + 1] - cs.sym_off[(size_t)b + i];
        longest = std::max(longest, l);
        same_len = same_len && l == cs.sym_off[(size_t)b + 1] - cs.sym_off[(size_t)b];
      }
      const char* suf = longest <= 4 ? "u" : "ull";       // symbols of <= 4 bytes: a 32-bit select chain
      for (int i = 0; i < ns; i++) {
        const uint32_t a0 = cs.sym_off[(size_t)b + i], a1 = cs.sym_off[(size_t)b + i + 1];
        uint64_t bits = 0;
        for (uint32_t j = a0; j < a1; j++) bits |= (uint64_t)cs.sym_data[j] << (8 * (j - a0));
        if (i + 1 < ns) { ls << "v == " << i << "u ? " << (a1 - a0) << "u : "; bs << "v == " << i << "u ? 0x" << std::hex << bits << std::dec << suf << " : "; }
        else { ls << (a1 - a0) << "u"; bs << "0x" << std::hex << bits << std::dec << suf; }
      }
      if (same_len) { ls.str(""); ls << longest << "u"; }
      o << "    if (b == " << b << ") { len = " << ls.str() << "; bits = (uint64_t)(" << bs.str() << "); return true; }\n";
    }
  }
  o << "    return false;\n  }\n";
  o << "  template <bool EMIT, bool CAREFUL, class Src, class Ctx>\n";
  o << "  static __device__ __forceinline__ void walk(const Ctx& c, const Src& src, Lane& L) {\n";
  int indent = 2;
  auto pad = [&]() { return std::string((size_t)indent * 2, ' '); };
  // Projection (walk_drop.h): an op of a dropped field runs counters-only over `dc`, the context view that discards them --
  // trusted in the emit walk's fast form.  Behind the last kept op the emit walk of a schema whose calls always have a size
  // pass stops: that pass has walked (and checked) the rest, and trailing bytes are ignored by contract.
  size_t stop_at = cs.prog.size();
  if (cs.projected) {
    bool any_drop = false;
    size_t last_kept = 0, end = 0;
    for (size_t i = 0; i < cs.prog.size() && cs.prog[i].code != OP_END; i++) {
      end = i + 1;
      if (cs.prog[i].flags & F_DROP) any_drop = true;
      else last_kept = i + 1;
    }
    if (any_drop) o << "    const DropCtx<Ctx, (EMIT && !CAREFUL)> dc(c);\n";
    if (last_kept < end && (cs.K > 0 || cs.size_always)) stop_at = last_kept;
  }
  // Head fusion (walk.h read_head LA): chains of statically adjacent heads.  la[i]: bit 0 = op i takes its head bytes from
  // the look-ahead, bit 1 = it leaves the look-ahead behind for the next one, bits 2.. = bytes the chain's first head reads.
  // A chain starts at a head-only op (nullable record / list branch, union index, int, non-nullable boolean / float, enum
  // index), runs through head-only ops and may END in a string; the first reading op of every variant of a union takes the
  // look-ahead the union index left.  It never crosses a loop boundary (LIST_NEXT / LIST_TAIL / LIST_END) and never needs
  // more than 8 bytes in the fast wire forms.  RUHVRO_HIP_NO_HEAD_FUSION=1: A/B knob.
  // Runs (wide schemas): `reps` repetitions of a pattern of `period` leaf ops of domain 0 whose ids (counter, buffers, node, enum
  // symbols) advance by constant steps -- a hundred nullable string columns, or (string, long, double) x 40 -- are emitted as
  // ONE loop over the pattern with the ids computed from the trip count, not as `reps x period` handler calls: the kernel's
  // size and hiprtc's time then follow the number of distinct column SHAPES, not the number of columns (a 97-column schema
  // unrolled took hiprtc 15 minutes).  Head fusion stays out of a run.  RUHVRO_HIP_NO_RUNS=1: A/B knob.
  struct Run { int period, reps; };
  std::map<size_t, Run> runs;
  std::vector<char> in_run(cs.prog.size(), 0);
  if (cs.wide && !std::getenv("RUHVRO_HIP_NO_RUNS")) {
    // (a defaulted leaf -- walk_resolve.h F_CONST -- names its own place in the default blob: never part of a run; a promoted leaf is
    //  a column shape of its own through its flags)
    auto leaf = [](const Op& q) { return q.dom == 0 && !(q.flags & F_CONST) && (q.code == OP_FIXED || q.code == OP_STRING || q.code == OP_ENUM || q.code == OP_BIN); };
    auto same_shape = [](const Op& x, const Op& y) {
      if (x.code != y.code || x.flags != y.flags || x.dom != y.dom) return false;
      if (x.code == OP_FIXED) return x.a == y.a;
      if (x.code == OP_ENUM) return x.c == y.c;
      if (x.code == OP_BIN) return x.a == y.a && x.b == y.b && x.c == y.c;
      return true;
    };
    auto step_ok = [](const Op& x0, const Op& x1, const Op& xr, const Op& xr1) {      // ids advance by the same steps from repetition to repetition
      return xr1.a - xr.a == x1.a - x0.a && xr1.b - xr.b == x1.b - x0.b && xr1.buf0 - xr.buf0 == x1.buf0 - x0.buf0 &&
             xr1.buf1 - xr.buf1 == x1.buf1 - x0.buf1 && xr1.buf2 - xr.buf2 == x1.buf2 - x0.buf2 && xr1.node - xr.node == x1.node - x0.node;
    };
    const size_t np = cs.prog.size();
    for (size_t i = 0; i < np && cs.prog[i].code != OP_END;) {
      int best_p = 0, best_m = 0;
      if (leaf(cs.prog[i])) {
        for (int p = 1; p <= 4; p++) {
          int m = 1;
          for (;; m++) {
            bool ok = true;
            for (int j = 0; j < p && ok; j++) {
              const size_t a = i + (size_t)(m - 1) * p + j, b = i + (size_t)m * p + j;
              ok = b < np && leaf(cs.prog[a]) && leaf(cs.prog[b]) && same_shape(cs.prog[i + j], cs.prog[b]) &&
                   step_ok(cs.prog[i + j], cs.prog[i + p + j], cs.prog[a], cs.prog[b]);
            }
            if (!ok) break;
          }
          if (m >= 3 && m * p >= 8 && m * p > best_m * best_p) { best_p = p; best_m = m; }
        }
      }
      if (best_p) {
        runs[i] = Run{best_p, best_m};
        for (size_t j = i; j < i + (size_t)best_p * best_m; j++) in_run[j] = 1;
        i += (size_t)best_p * best_m;
      } else {
        i++;
      }
    }
  }
  std::vector<int> la(cs.prog.size(), 0);
  if (!std::getenv("RUHVRO_HIP_NO_HEAD_FUSION")) {
    const size_t nprog = cs.prog.size();
    auto head_bytes = [&](const Op& q) -> int {      // worst-case bytes of the head in its fast wire form; 0 = not fusable
      if (in_run[(size_t)(&q - cs.prog.data())]) return 0;
      if (q.flags & F_CONST) return 0;                  // (a defaulted leaf reads the default blob, not the record: no chain crosses it)
      const int b = (q.flags & F_NULLABLE) ? 1 : 0;
      switch (q.code) {
        case OP_REC_BEGIN: return 1;
        case OP_LIST_BEGIN: return (q.flags & F_NULLABLE) ? 1 : 0;
        case OP_UNION_BEGIN: return 2;
        case OP_ENUM: return b + 2;
        case OP_STRING: return b + (variant_on("LEN16") ? 2 : 3);   // (walk.h: lengths take the 3-byte form, indices the 2-byte one, an int 5 bytes)
        case OP_FIXED:
          if (q.a == FK_I32) return b + (variant_on("INT28") ? 4 : 5);
          if (q.a == FK_BOOL) return b ? 0 : 1;
          if (q.a == FK_F32) return b ? 0 : 4;
          return 0;                                   // long / double: up to 8 bytes and more
        default: return 0;
      }
    };
    auto in_a_run = [&](const Op& q) { return in_run[(size_t)(&q - cs.prog.data())] != 0; };
    auto head_only = [&](const Op& q) { return q.code != OP_STRING && head_bytes(q) > 0 && !in_a_run(q); };
    auto loop_edge = [&](const Op& q) { return q.code == OP_LIST_NEXT || q.code == OP_LIST_TAIL || q.code == OP_LIST_END || q.code == OP_END; };
    auto passive = [&](const Op& q) { return q.code == OP_REC_END || q.code == OP_UNION_END; };
    size_t i = 0;
    while (i < nprog && cs.prog[i].code != OP_END) {
      if (la[i] || !head_only(cs.prog[i])) { i++; continue; }
      // grow a chain from op i
      std::vector<size_t> chain{i};
      int used = head_bytes(cs.prog[i]);
      size_t cur = i;
      for (;;) {
        const Op& a = cs.prog[cur];
        if (a.code == OP_UNION_BEGIN) {
          // every variant's first reading op consumes; the chain ends here
          int worst = 0;
          std::vector<size_t> cons;
          size_t j = cur + 1;
          int depth = 0;
          bool fresh = false, ok = true;
          for (; j < nprog; j++) {
            const Op& q = cs.prog[j];
            if (q.code == OP_UNION_END && depth == 0) break;
            if (q.code == OP_UNION_BEGIN) depth++;
            if (q.code == OP_UNION_END) depth--;
            if (depth == 0 && q.code == OP_VARIANT) { fresh = true; continue; }
            if (fresh && depth <= 1) {
              fresh = false;
              if (q.code == OP_VARIANT) { fresh = true; continue; }
              const int hb = head_bytes(q);
              if (hb > 0 && !loop_edge(q) && q.code != OP_LIST_BEGIN) { cons.push_back(j); worst = std::max(worst, hb); }
            }
          }
          if (ok && !cons.empty() && used + worst <= 8) {
            for (size_t c : cons) la[c] |= 1;
            la[cur] |= 2;
            used += worst;
          }
          break;
        }
        size_t j = cur + 1;
        while (j < nprog && passive(cs.prog[j])) j++;
        if (j >= nprog || loop_edge(cs.prog[j])) break;
        const Op& b = cs.prog[j];
        const int hb = head_bytes(b);
        if (hb == 0 || used + hb > 8 || la[j]) break;
        if (b.code == OP_LIST_BEGIN && !(b.flags & F_NULLABLE)) break;
        la[cur] |= 2;
        la[j] |= 1;
        used += hb;
        chain.push_back(j);
        if (!head_only(b)) break;                       // a string ends the chain (its body follows)
        cur = j;
      }
      if (la[i] & 2) la[i] |= (used <= 4 ? 4 : 8) << 2;
      i++;
    }
  }
  // one op as a handler call; E / CF are the EMIT / CAREFUL template arguments in the generated text, cx / ln the context and lane
  auto leaf_call = [&](const Op& p, const std::string& E, const std::string& CF, const std::string& cx, const std::string& ln) {
    std::ostringstream lit;
    lit << "{" << op_name(p.code) << ", " << p.flags << ", " << p.dom << ", " << p.a << ", " << p.b << ", " << p.c << ", "
        << p.buf0 << ", " << p.buf1 << ", " << p.buf2 << ", " << p.node << "}";
    const std::string decl = "constexpr Op op = " + lit.str() + "; ";
    const std::string args = "<" + E + ", " + CF + ">(" + cx + ", src, " + ln + ", op); }\n";
    if (p.flags & F_CONST) return "{ " + decl + "run_const" + args;
    switch (p.code) {
      case OP_FIXED: return "{ " + decl + ((p.flags & F_PROMOTE_MASK) ? "h_fixed_p" : "h_fixed") + args;
      case OP_STRING:
      case OP_ENUM: return "{ " + decl + "h_string" + args;
      case OP_REC_BEGIN: return "{ " + decl + "h_rec_begin" + args;
      case OP_REC_END: return std::string("h_rec_end(") + ln + ");\n";
      case OP_UNION_BEGIN: return "{ " + decl + "h_union_begin" + args;
      case OP_VARIANT: return "{ " + decl + "h_variant(" + ln + ", op); }\n";
      case OP_BIN: return "{ " + decl + "h_bin" + args;
      case OP_UNION_END: return std::string("h_union_end(") + ln + ");\n";
      default: return std::string();
    }
  };
  int list_depth = 0, leaves = 0;      // (wide schemas: a top-up hook behind every few leaf ops outside the lists)
  const int topup_every = [] { const char* e = std::getenv("RUHVRO_HIP_TOPUP_EVERY"); const int v = e ? std::atoi(e) : 0; return v > 0 ? v : 2; }();
  for (size_t i = 0; i < cs.prog.size(); i++) {
    const Op& p = cs.prog[i];
    if (p.code == OP_END) break;
    if (i == stop_at) o << pad() << "if constexpr (EMIT) return;      // only dropped fields from here on\n";
    if (runs.count(i)) {       // a run: one loop over its pattern, ids from the trip count
      const Run rn = runs.at(i);
      o << pad() << "_Pragma(\"nounroll\") for (int r = 0; r < " << rn.reps << "; r++) {\n";
      indent++;
      if (cs.wide) o << pad() << "h_topup(c, src, L);\n";      // (lane windows / a sliding window: kept under the cursors, walk.h)
      for (int j = 0; j < rn.period; j++) {
        const Op& q0 = cs.prog[i + (size_t)j], & q1 = cs.prog[i + (size_t)rn.period + (size_t)j];
        auto fld = [&](int v0, int v1) { std::ostringstream f; f << v0; if (v1 != v0) f << " + r * " << (v1 - v0); return f.str(); };
        o << pad() << "{ const Op op = {" << op_name(q0.code) << ", " << q0.flags << ", " << q0.dom << ", " << fld(q0.a, q1.a) << ", " << fld(q0.b, q1.b)
          << ", " << q0.c << ", " << fld(q0.buf0, q1.buf0) << ", " << fld(q0.buf1, q1.buf1) << ", " << fld(q0.buf2, q1.buf2) << ", " << fld(q0.node, q1.node) << "}; ";
        const char* targs = (q0.flags & F_DROP) ? "<false, CAREFUL>(dc, src, L, op); }\n" : "<EMIT, CAREFUL>(c, src, L, op); }\n";
        switch (q0.code) {
          case OP_FIXED: o << ((q0.flags & F_PROMOTE_MASK) ? "h_fixed_p" : "h_fixed") << targs; break;
          case OP_BIN: o << "h_bin" << targs; break;
          default: o << "h_string" << targs; break;
        }
      }
      indent--;
      o << pad() << "}\n";
      i += (size_t)rn.period * rn.reps - 1;
      continue;
    }
    std::ostringstream lit;
    lit << "{" << op_name(p.code) << ", " << p.flags << ", " << p.dom << ", " << p.a << ", " << p.b << ", " << p.c << ", "
        << p.buf0 << ", " << p.buf1 << ", " << p.buf2 << ", " << p.node << "}";
    const std::string decl = "constexpr Op op = " + lit.str() + "; ";
    if (p.code == OP_LIST_NEXT && dense.count(i - 1)) {
      // the trusted fast walk of the emit kernel handles this list one lane per item; every other walk keeps the block loop
      size_t end = i + 1;
      while (cs.prog[end].code != OP_LIST_TAIL) end++;
      // (the fast size walk over a SlideSrc -- the ranged kernels -- sizes the list of a record larger than the window by the
      //  wavefront-parallel item scan, spec_body.h giant_list_size; the block loop behind it then finds that lane done)
      o << pad() << "if constexpr (!EMIT && !CAREFUL && Ctx::kDense && Src::kSlide) {\n";
      indent++;
      o << pad() << "auto body = [&](auto em, const auto& cc, Lane& LL) {\n";
      indent++;
      for (size_t j = i + 1; j < end; j++) o << pad() << leaf_call(cs.prog[j], "false", "false", "cc", "LL");
      indent--;
      o << pad() << "};\n";
      o << pad() << "giant_list_size<Spec, " << dense.at(i - 1) << ", " << (p.a - 1) << ", " << p.c << ">(c, src, L, body);\n";
      indent--;
      o << pad() << "}\n";
      o << pad() << "if constexpr (EMIT && !CAREFUL && Ctx::kDense) {\n";
      indent++;
      o << pad() << "auto body = [&](auto em, const auto& cc, Lane& LL) {\n";
      indent++;
      o << pad() << "constexpr bool E = decltype(em)::value != 0;\n";
      for (size_t j = i + 1; j < end; j++) o << pad() << leaf_call(cs.prog[j], "E", "false", "cc", "LL");
      indent--;
      o << pad() << "};\n";
      o << pad() << "dense_list<Spec, " << dense.at(i - 1) << ", " << (p.a - 1) << ", " << p.c << ">(c, src, L, body);\n";
      indent--;
      o << pad() << "} else\n";
    }
    const bool dr = (p.flags & F_DROP) != 0;
    const std::string E = dr ? "false" : "EMIT", cx = dr ? "dc" : "c";
    const std::string tp = "<" + E + ", CAREFUL" + (la[i] ? ", " + std::to_string(la[i]) : std::string()) + ">";
    if (p.flags & F_CONST) {
      o << pad() << "{ " << decl << "run_const<EMIT, CAREFUL>(c, src, L, op); }\n";
    } else
    switch (p.code) {
      case OP_FIXED: o << pad() << "{ " << decl << ((p.flags & F_PROMOTE_MASK) ? "h_fixed_p" : "h_fixed") << tp << "(" << cx << ", src, L, op); }\n"; break;
      case OP_STRING:
      case OP_ENUM: o << pad() << "{ " << decl << "h_string" << tp << "(" << cx << ", src, L, op); }\n"; break;
      case OP_REC_BEGIN: o << pad() << "{ " << decl << "h_rec_begin" << tp << "(" << cx << ", src, L, op); }\n"; break;
      case OP_REC_END: o << pad() << "h_rec_end(L);\n"; break;
      case OP_UNION_BEGIN: o << pad() << "{ " << decl << "h_union_begin" << tp << "(" << cx << ", src, L, op); }\n"; break;
      case OP_VARIANT: o << pad() << "{ " << decl << "h_variant(L, op); }\n"; break;
      case OP_BIN: o << pad() << "{ " << decl << "h_bin<" << E << ", CAREFUL>(" << cx << ", src, L, op); }\n"; break;
      case OP_UNION_END: o << pad() << "h_union_end(L);\n"; break;
      case OP_LIST_BEGIN: o << pad() << "{ " << decl << "h_list_begin" << tp << "(" << cx << ", src, L, op); }\n"; break;
      case OP_LIST_NEXT:
        o << pad() << "for (;;) {\n";
        indent++;
        o << pad() << "{ " << decl << "if (!h_list_next<CAREFUL, (EMIT && !CAREFUL)>(" << cx << ", src, L, op)) break; }\n";
        break;
      case OP_LIST_TAIL:
        o << pad() << "{ " << decl << "h_list_tail(" << cx << ", L, op); }\n";
        indent--;
        o << pad() << "}\n";
        break;
      case OP_LIST_END: o << pad() << "{ " << decl << "h_list_end<" << E << ">(" << cx << ", L, op); }\n"; break;
      default: break;
    }
    if (p.code == OP_LIST_NEXT) list_depth++;
    if (p.code == OP_LIST_TAIL) list_depth--;
    if (cs.wide && list_depth == 0 && (p.code == OP_FIXED || p.code == OP_STRING || p.code == OP_ENUM || p.code == OP_BIN || p.code == OP_LIST_END) &&
        (++leaves % topup_every) == 0)
      o << pad() << "h_topup(c, src, L);\n";
  }
  o << "  }\n};\n";
  // (each kernel is its own hiprtc program when the engine compiles in the background -- kernel_jobs.cpp: `parts` selects the entries)
  if (parts & (1u << KP_SIZE))
  o << "extern \"C\" __global__ void __launch_bounds__(" << spec_tile_records(cs) << ") rh_spec_size(KParams P) { spec_size<Spec>(P); }\n";
  // the emit kernel is held to 128 VGPRs (4 waves per SIMD): one register more and a CU runs 12 instead of 16 of its waves
  // (measured in round 3 with an experimental kernel at 129 VGPRs: k_emit 0.90 -> 1.06 ms whatever its LDS budget, profiles/r03a_*)
  if (parts & (1u << KP_EMIT))
    o << "extern \"C\" __global__ void __launch_bounds__(" << spec_tile_records(cs) << ") __attribute__((amdgpu_waves_per_eu(4, 8))) rh_spec_emit(KParams P) { " << (flat ? "spec_emit_flat" : "spec_emit") << "<Spec>(P); }\n";
  // the single-pass form (spec_body.h spec_fused): sizes, scans across tiles (look-back) and emits in one launch
  if (cs.K <= 64 && (parts & (1u << KP_FUSED)))      // (the look-back wave holds one lane per counter)
    o << "extern \"C\" __global__ void __launch_bounds__(" << spec_tile_records(cs) << ") __attribute__((amdgpu_waves_per_eu(4, 8))) rh_spec_fused(KParams P) { spec_fused<Spec>(P); }\n";
  // the ranged pair (spec_body.h ranged_tile): the tiles that do not fit the LDS window
  if (parts & (1u << KP_SIZE_R))
    o << "extern \"C\" __global__ void __launch_bounds__(" << spec_tile_records(cs) << ") rh_spec_size_r(KParams P) { spec_size<Spec, true>(P); }\n";
  if (parts & (1u << KP_EMIT_R))
    // (a wide schema's window leaves a CU eight one-wavefront workgroups -- two per SIMD: its ranged emit kernel may use the
    //  256 VGPRs that leaves; held to 128 it spilled 105 of them to scratch memory)
    o << "extern \"C\" __global__ void __launch_bounds__(" << spec_tile_records(cs) << ") __attribute__((amdgpu_waves_per_eu(" << (cs.wide ? "2, 4" : "4, 8")
      << "))) rh_spec_emit_r(KParams P) { " << (flat ? "spec_emit_flat" : "spec_emit") << "<Spec, true>(P); }\n";
  o << "}  // namespace rh\n";
  return o.str();
}

// ---------------------------------------------------------------------------
// Arrow -> Avro: the same schema program, unrolled over encode_walk.h's handlers
// ---------------------------------------------------------------------------
namespace {
bool enc_loads(int code) {
  return code == OP_FIXED || code == OP_STRING || code == OP_ENUM || code == OP_REC_BEGIN || code == OP_UNION_BEGIN ||
         code == OP_LIST_BEGIN || code == OP_BIN;
}
constexpr int kEncFetchBatch = 4;   // strings whose bytes are requested together (4-8 VGPRs each; 6 and 8 cost a wave per SIMD)
constexpr int kEncLoadGroup = 32;   // loads kept in flight together per row domain (bounds VGPR pressure on wide schemas)
}  // namespace

std::string generate_encode_source(const CompiledSchema& cs, unsigned parts) {
  std::ostringstream o;
  o << "// generated by ruhvro_hip specialize.cpp (encode) -- do not edit\n";
  emit_variant_defines(o);
  bool profile = false;
  if (const char* e = std::getenv("RUHVRO_HIP_PROFILE"))
    if (*e && *e != '0') profile = true;
  if (profile) o << "#define RH_PROFILE 1\n";
  int mark = 2;     // phase slots 2..19: the stretches of the walk between list loops
  o << "#include \"encode_spec.h\"\n";
  o << "namespace rh {\n";
  o << "struct ESpec {\n";
  o << "  static constexpr int NDOM = " << cs.ndom << ", DEPTH = " << cs.list_depth << ";\n";
  const size_t nops = cs.prog.size();
  // load groups: the loading ops of one row domain, in program order, kEncLoadGroup at a time; a group's loads are
  // issued right before its first op runs (all ops of a domain sit at one brace level: the body of its list)
  std::vector<int> group_of(nops, -1);
  std::vector<std::vector<size_t>> groups;
  {
    std::map<int, int> open;      // dom -> index of its group still being filled
    for (size_t i = 0; i < nops; i++) {
      const Op& p = cs.prog[i];
      if (p.code == OP_END) break;
      if (!enc_loads(p.code)) continue;
      auto it = open.find(p.dom);
      if (it == open.end() || groups[(size_t)it->second].size() >= (size_t)kEncLoadGroup) {
        groups.emplace_back();
        open[p.dom] = (int)groups.size() - 1;
        it = open.find(p.dom);
      }
      groups[(size_t)it->second].push_back(i);
      group_of[i] = it->second;
    }
  }
  // second-level loads (string bytes, enum symbol text) of a group: requested kEncFetchBatch strings at a time, a batch
  // right before its first put, so the strings of a batch share one HBM round trip instead of paying one each
  auto small_enum = [&](const Op& p) {
    bool small = p.c > 0;
    for (int sidx = 0; sidx < p.c; sidx++)
      if (cs.sym_off[(size_t)p.b + sidx + 1] - cs.sym_off[(size_t)p.b + sidx] > 16) small = false;
    return small;
  };
  std::vector<char> fetched(nops, 0);
  std::map<size_t, std::vector<size_t>> batch_at;      // first op of a batch -> the batch
  for (size_t g = 0; g < groups.size(); g++) {
    std::vector<size_t> cur;
    for (size_t j : groups[g]) {
      const Op& p = cs.prog[j];
      if (p.code != OP_STRING && !(p.code == OP_ENUM && small_enum(p))) continue;
      fetched[j] = 1;
      cur.push_back(j);
      if (cur.size() == (size_t)kEncFetchBatch) { batch_at[cur.front()] = cur; cur.clear(); }
    }
    if (!cur.empty()) batch_at[cur.front()] = cur;
  }
  o << "  template <int MODE, class Ctx>\n";
  o << "  static __device__ __forceinline__ void walk(Ctx& c, ELane& L) {\n";
  for (size_t i = 0; i < nops; i++) {
    const Op& p = cs.prog[i];
    if (p.code == OP_END) break;
    o << "    constexpr Op op" << i << " = {" << op_name(p.code) << ", " << p.flags << ", " << p.dom << ", " << p.a << ", "
      << p.b << ", " << p.c << ", " << p.buf0 << ", " << p.buf1 << ", " << p.buf2 << ", " << p.node << "};\n";
  }
  int indent = 2;
  auto pad = [&]() { return std::string((size_t)indent * 2, ' '); };
  auto emit_fetches = [&](const std::vector<size_t>& batch) {
    for (size_t j : batch) {
      const Op& q = cs.prog[j];
      if (q.code == OP_STRING && q.dom == 0) {          // rows of domain 0: cooperative, through the wave's LDS staging area
        o << pad() << "const StrF d" << j << " = e_string_cofetch<MODE>(c, op" << j << ", v" << j << ");\n";
      } else if (q.code == OP_STRING) {
        o << pad() << "const Str32 d" << j << " = e_string_fetch<MODE>(c, op" << j << ", v" << j << ");\n";
      } else {
        uint32_t longest = 0;
        for (int sidx = 0; sidx < q.c; sidx++)
          longest = std::max<uint32_t>(longest, cs.sym_off[(size_t)q.b + sidx + 1] - cs.sym_off[(size_t)q.b + sidx]);
        o << pad() << "const v4w d" << j << " = e_enum_fetch_n<" << longest << ">(c, op" << j << ", v" << j << ");\n";
      }
    }
  };
  // Software-pipelined list bodies: an item costs the walk two DEPENDENT round trips (its offsets / values, then its string
  // bytes).  The first-level loads of item i + 1 do not depend on item i -- the next item is the next row of the child
  // domain -- so they are issued at the top of iteration i, next to item i's byte fetches: one exposed round trip per
  // iteration instead of two, with the same loads.  pipe[g]: group g is the first load group of a list body.
  // RUHVRO_HIP_NO_ENC_PIPE=1: A/B knob.
  std::vector<char> pipe(groups.size(), 0);
  std::vector<int> pipe_depth(groups.size(), 0);      // nesting depth of the list (its slot of the items-left counters)
  std::map<size_t, int> pipe_at_next;       // index of a LIST_NEXT -> the group preloaded in front of its loop
  if (!std::getenv("RUHVRO_HIP_NO_ENC_PIPE")) {
    for (size_t i = 0; i + 1 < nops; i++) {
      if (cs.prog[i].code != OP_LIST_BEGIN || cs.prog[i + 1].code != OP_LIST_NEXT) continue;
      const int child = cs.prog[i].a;
      for (size_t j = i + 2; j < nops && !(cs.prog[j].code == OP_LIST_END && cs.prog[j].a == child); j++) {
        if (group_of[j] < 0 || cs.prog[j].dom != child) continue;
        if (groups[(size_t)group_of[j]].front() == j) { pipe[(size_t)group_of[j]] = 1; pipe_depth[(size_t)group_of[j]] = cs.prog[i].c; pipe_at_next[i + 1] = group_of[j]; }
        break;
      }
    }
  }
  // ... and the FIRST item's first-level loads of a top-level list go out as soon as the row's own loads are back (its child
  // rows start at the list's offset), next to the row's string fetches, instead of costing the loop a round trip of its own.
  // hoisted[lb]: the LIST_BEGIN whose body group is preloaded at its own group's front.  RUHVRO_HIP_NO_ENC_HOIST=1: A/B knob.
  std::map<size_t, std::vector<size_t>> hoist_at;      // front op of a group -> the LIST_BEGINs of that group to preload for
  std::vector<char> hoisted(nops, 0);
  if (!std::getenv("RUHVRO_HIP_NO_ENC_HOIST")) {
    for (const auto& kv : pipe_at_next) {
      const size_t lb = kv.first - 1;
      if (cs.prog[lb].dom != 0 || group_of[lb] < 0) continue;
      hoist_at[groups[(size_t)group_of[lb]].front()].push_back(lb);
      hoisted[lb] = 1;
    }
  }
  auto load_expr = [&](size_t j, const std::string& ahead) -> std::string {
    const int code = cs.prog[j].code;
    const std::string a = "(c, op" + std::to_string(j) + ahead + ")";
    if (code == OP_FIXED) return "e_fixed_load" + a;
    if (code == OP_REC_BEGIN) return "e_rec_load" + a;
    if (code == OP_UNION_BEGIN) return "e_union_load" + a;
    if (code == OP_BIN) return "e_bin_load" + a;
    return "e_span_load" + a;
  };
  auto load_type = [&](size_t j) -> const char* {
    const int code = cs.prog[j].code;
    return code == OP_FIXED ? "FixedV" : code == OP_REC_BEGIN ? "bool" : code == OP_UNION_BEGIN ? "int32_t" : code == OP_BIN ? "BinV" : "SpanV";
  };
  for (size_t i = 0; i < nops; i++) {
    const Op& p = cs.prog[i];
    if (p.code == OP_END) break;
    if (group_of[i] >= 0 && groups[(size_t)group_of[i]].front() == i) {
      const std::vector<size_t>& grp = groups[(size_t)group_of[i]];
      if (pipe[(size_t)group_of[i]]) {
        for (size_t j : grp) o << pad() << "const " << load_type(j) << " v" << j << " = nv" << j << ";\n";
        // (a lane on its last item -- or on none -- asks for its current row again: row + 1 may lie behind the column, where an
        //  offsets slot holds padding, and the byte fetch of the next iteration is unconditional)
        const std::string ahead = ", c.rem(" + std::to_string(pipe_depth[(size_t)group_of[i]]) + ") > 1u ? 1u : 0u";
        for (size_t j : grp) o << pad() << "nv" << j << " = " << load_expr(j, ahead) << ";      // the next item's\n";
      } else {
        for (size_t j : grp) o << pad() << "const " << load_type(j) << " v" << j << " = " << load_expr(j, "") << ";\n";
      }
    }
    {
      auto it = batch_at.find(i);
      if (it != batch_at.end()) emit_fetches(it->second);
    }
    {
      auto it = hoist_at.find(i);
      if (it != hoist_at.end())
        for (size_t lb : it->second)
          for (size_t j : groups[(size_t)pipe_at_next.at(lb + 1)])      // (the child cursor is still 0: `ahead` is the absolute row)
            o << pad() << load_type(j) << " nv" << j << " = " << load_expr(j, ", v" + std::to_string(lb) + ".s0") << ";\n";
    }
    switch (p.code) {
      case OP_FIXED: o << pad() << "e_fixed_put<MODE>(c, L, op" << i << ", v" << i << ");\n"; break;
      case OP_BIN: o << pad() << "e_bin_put<MODE>(c, L, op" << i << ", v" << i << ");\n"; break;
      case OP_STRING:
        if (p.dom == 0) o << pad() << "e_string_put_cf<MODE>(c, L, op" << i << ", v" << i << ", d" << i << ");\n";
        else o << pad() << "e_string_put_pf<MODE>(c, L, op" << i << ", v" << i << ", d" << i << ");\n";
        break;
      case OP_ENUM: {
        // symbols of at most 16 bytes are matched against constants folded into the kernel (length + masked dwords
        // of the prefetched symbol text); longer ones go through the symbol table in HBM
        if (!fetched[i]) {
          o << pad() << "e_enum_put<MODE>(c, L, op" << i << ", v" << i << ", " << i
            << ", EnumTableFinder{c.sym_off, c.sym_data, op" << i << ".b, op" << i << ".c});\n";
          break;
        }
        o << pad() << "e_enum_put_pf<MODE>(c, L, op" << i << ", v" << i << ", " << i << ", d" << i
          << ", [](const v4w a, uint32_t n) -> int32_t {\n";
        indent++;
        for (int sidx = 0; sidx < p.c; sidx++) {
          const uint32_t a0 = cs.sym_off[(size_t)p.b + sidx], a1 = cs.sym_off[(size_t)p.b + sidx + 1];
          const uint32_t len = a1 - a0;
          o << pad() << "if (n == " << len << "u";
          static const char* comp[] = {"a.x", "a.y", "a.z", "a.w"};
          for (uint32_t d = 0; d * 4 < len; d++) {
            uint32_t want = 0, mask = 0;
            for (uint32_t j = 0; j < 4 && d * 4 + j < len; j++) {
              want |= (uint32_t)cs.sym_data[a0 + d * 4 + j] << (8 * j);
              mask |= 0xFFu << (8 * j);
            }
            char buf[96];
            if (mask == 0xFFFFFFFFu) std::snprintf(buf, sizeof buf, " && %s == 0x%08xu", comp[d], want);
            else std::snprintf(buf, sizeof buf, " && (%s & 0x%08xu) == 0x%08xu", comp[d], mask, want);
            o << buf;
          }
          o << ") return " << sidx << ";\n";
        }
        o << pad() << "return -1;\n";
        indent--;
        o << pad() << "});\n";
        break;
      }
      case OP_REC_BEGIN: o << pad() << "e_rec_begin<MODE>(c, L, op" << i << ", v" << i << ");\n"; break;
      case OP_REC_END: o << pad() << "e_rec_end(L);\n"; break;
      case OP_UNION_BEGIN: o << pad() << "e_union_begin<MODE>(c, L, op" << i << ", v" << i << ", " << i << ");\n"; break;
      case OP_VARIANT: o << pad() << "e_variant(L, op" << i << ");\n"; break;
      case OP_UNION_END: o << pad() << "e_union_end(L);\n"; break;
      case OP_LIST_BEGIN:
        if (profile && indent == 2 && mark < 19) o << pad() << "L.clk.mark(" << mark++ << ");\n";
        o << pad() << "e_list_begin<MODE>(c, L, op" << i << ", v" << i << ");\n";
        break;
      case OP_LIST_NEXT: {
        auto pit = pipe_at_next.find(i);
        if (pit != pipe_at_next.end() && !hoisted[i - 1])      // the first item's first-level loads, in front of the loop
          for (size_t j : groups[(size_t)pit->second]) o << pad() << load_type(j) << " nv" << j << " = " << load_expr(j, "") << ";\n";
        o << pad() << "for (;;) {\n";
        indent++;
        o << pad() << "if (!e_list_next(c, L, op" << i << ")) break;\n";
        break;
      }
      case OP_LIST_TAIL:
        o << pad() << "e_list_tail(c, L, op" << i << ");\n";
        indent--;
        o << pad() << "}\n";
        break;
      case OP_LIST_END:
        o << pad() << "e_list_end<MODE>(c, L);\n";
        if (profile && indent == 2 && mark < 19) o << pad() << "L.clk.mark(" << mark++ << ");\n";
        break;
      default: break;
    }
  }
  if (profile) o << "    L.clk.mark(19);\n";
  o << "  }\n};\n";
  if (parts & (1u << KP_ESIZE))
    o << "extern \"C\" __global__ void __launch_bounds__(256) rh_espec_size(EParams P) {\n"
    << "  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];\n  e_size_body<ESpecW<ESpec>>(P, smem);\n}\n";
  if (parts & (1u << KP_EEMIT))
    o << "extern \"C\" __global__ void __launch_bounds__(256) rh_espec_emit(EParams P) {\n"
    << "  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];\n  e_emit_body<ESpecW<ESpec>>(P, smem);\n}\n";
  o << "}  // namespace rh\n";
  return o.str();
}

bool schema_has_lean(const CompiledSchema& cs) { return (cs.K > 0 || cs.size_always) && !cs.wide; }

std::string generate_lean_source(const CompiledSchema& cs, unsigned parts) {
  if (!schema_has_lean(cs)) return "";
  struct Scope { Scope() { t_lean = true; } ~Scope() { t_lean = false; } } lean;
  return generate_kernel_source(cs, parts);
}

std::string generate_part_source(const CompiledSchema& cs, int part) {
  if (part < 0 || part >= KP_COUNT) return "";
  if (part == KP_SIZE_L || part == KP_EMIT_L) return generate_lean_source(cs, 1u << (part == KP_SIZE_L ? KP_SIZE : KP_EMIT));
  if (part == KP_FUSED && cs.K > 64) return "";
  if (kernel_part_is_encode(part)) return (cs.encode_unsupported.empty() && !cs.projected) ? generate_encode_source(cs, 1u << part) : std::string();      // (projection is decode only)
  return generate_kernel_source(cs, 1u << part);
}

}  // namespace rh
