/* ruhvro_hip.h -- C ABI of the MI355X-native Avro -> Arrow direct-decode engine.
 *
 * Drop-in boundary for ONE path of Tyler-Sch/pyruhvro: the chunked direct
 * decode that `pyruhvro.deserialize_array_threaded` reaches.  Each entry point
 * names the reference interface it replaces (paths relative to the reference
 * repository root).  Plain pointers and sizes only; no torch / pybind types.
 *
 * Conventions: functions returning int return 0 on success; on failure they
 * return non-zero and, when `err` is non-NULL, store a malloc'd NUL-terminated
 * message in *err (release with rh_free_string).  Decode errors carry exactly
 * the reference's message text (ruhvro/src/fast_decode.rs:575,591,634,646,
 * 849,866,874,884,898,906,910); the Python layer maps them to ValueError as
 * src/lib.rs:25-27 does.  All functions are thread-safe; a compiled schema
 * may be shared by concurrent calls.
 */
#ifndef RUHVRO_HIP_H
#define RUHVRO_HIP_H
#include <stddef.h>
#include <stdint.h>
#include "arrow_c_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RH_ABI_VERSION 7

/* error classes (return codes) */
#define RH_OK 0
#define RH_ERR_SCHEMA 1      /* schema JSON invalid / outside the direct-decode subset */
#define RH_ERR_DECODE 2      /* malformed Avro datum: reference message text in *err  */
#define RH_ERR_RUNTIME 3     /* HIP / allocation failure                               */
#define RH_ERR_ARGUMENT 4

typedef struct rh_schema rh_schema;

/* Replaces ruhvro::deserialize::parse_schema (ruhvro/src/deserialize.rs:18-20)
 * plus the per-call schema work of the fast path: the is_supported gate
 * (ruhvro/src/fast_decode.rs:38-61), to_arrow_schema
 * (ruhvro/src/schema_translate.rs:19-37) and decoder-tree construction
 * (fast_decode.rs:176-414).  The result is immutable; cache it by schema
 * string as src/lib.rs:39-54 does. */
rh_schema* rh_schema_compile(const char* json, size_t len, char** err);
void rh_schema_free(rh_schema* s);

/* Column projection (decode only).  A new, independent, immutable rh_schema that decodes the same Avro records into the
 * top-level columns names[0..n_names) only, in THAT order: every decode entry point then returns exactly what the full
 * schema's call followed by RecordBatch.select(names) returns -- buffer for buffer, field metadata included -- without
 * building, copying or exporting the other columns.  A dropped field is still walked (wire order is field order) with the
 * size walk's checks, so a malformed record raises the full decode's message for the lowest failing record even when
 * the damaged bytes belong to a dropped field.  Names are distinct top-level field names; a record / union / array / map
 * column is taken whole or not at all (a dotted path is refused).  NULL + RH_ERR_SCHEMA-style message in *err for an
 * empty list, an unknown, duplicate or dotted name.  The result has its own size history and its own specialised
 * kernels (its generated source differs, so does rh_schema_kernel_key) and is accepted by rh_schema_export, rh_decode,
 * rh_decode_packed, rh_decode_device (RH_ASYNC / RH_SINGLE_PASS / multi-device forms included), rh_schema_prebuild
 * (decode kernels only), rh_schema_kernels_ready, rh_schema_kernel_source and rh_schema_kernel_key; rh_encode /
 * rh_encode_device refuse it with RH_ERR_ARGUMENT.  Free it with rh_schema_free; it does not reference `s`.
 * Added WITHOUT a change of RH_ABI_VERSION (7): a caller discovers it by the presence of the symbol (dlsym). */
rh_schema* rh_schema_project(const rh_schema* s, const char* const* names, uint32_t n_names, char** err);

/* Reader schemas (strict decode only).  A new, independent, immutable rh_schema that decodes records WRITTEN with `writer`
 * into the columns of the Avro schema `reader_json` (Avro 1.11 "Schema Resolution", restricted): every decode entry point
 * returns, buffer for buffer and with the reader's Arrow schema (field metadata included), what a plain decode under the
 * reader schema gives for the same values as a writer of the reader schema would have encoded them.
 *   top level:  both records have the same unqualified name; fields are matched by name only (no aliases); a writer field the
 *               reader lacks is walked and not built; columns are in the reader's order; a reader field the writer lacks
 *               needs a `default` -- null (a union whose first branch is null), boolean, int, long, float, double, string,
 *               bytes or an enum symbol; a union default belongs to the first branch -- and holds it in every row.
 *   any depth:  promotions int -> long / float / double, long -> float / double, float -> double (the C cast: one rounding),
 *               string <-> bytes (the Arrow type only).  Everything else must match structurally (nested records field for
 *               field, enums symbol for symbol, union branches place for place).
 * NULL and a message that starts with "reader schema: " and names the field for anything else: a missing or unsupported
 * default (record / array / map / fixed), nested record evolution, a union against a non-union, differing enum symbols, a
 * pair that is no promotion.  A malformed record raises the plain `writer` decode's message for the lowest failing record,
 * also when the damage is in a field the reader lacks.  `writer` is a schema of rh_schema_compile.  The result has its own
 * size history and specialised kernels and is accepted by rh_schema_export, rh_decode, rh_decode_packed, rh_decode_device
 * (RH_ASYNC and the multi-device forms included; RH_SINGLE_PASS runs the fused kernel, which handles the new ops, with the
 * same buffers), rh_schema_prebuild, rh_schema_kernels_ready, rh_schema_kernel_source and rh_schema_kernel_key.  rh_encode*,
 * rh_validate*, rh_decode*_tolerant and rh_schema_placeholder refuse it with RH_ERR_ARGUMENT.  A reader text equal to the
 * writer's gives a plain compile of the writer.  Free it with rh_schema_free; it does not reference `writer`.
 * Added WITHOUT a change of RH_ABI_VERSION (7): a caller discovers it by the presence of the symbol (dlsym). */
rh_schema* rh_schema_resolve(const rh_schema* writer, const char* reader_json, size_t len, char** err);

/* Arrow schema of the produced batches, exported as a "+s" struct schema whose
 * children are the batch columns (what arrow-rs hands pyarrow at
 * src/lib.rs:70,88 through its pyarrow FFI).  Caller releases out->release. */
int rh_schema_export(const rh_schema* s, struct ArrowSchema* out);

/* clamp_chunks (ruhvro/src/deserialize.rs:53-55): number of batches a decode
 * of n records with `num_chunks` returns. */
uint32_t rh_clamp_chunks(uint64_t n, uint64_t num_chunks);

/* The multi-GPU deal (see rh_opts.devices): shard `shard` of `n_shards` owns chunks [*chunk_lo, *chunk_hi) of the
 * k = rh_clamp_chunks(n, num_chunks) reference chunks, i.e. rows [*row_lo, *row_hi) (build_slices,
 * deserialize.rs:57-68: k-1 chunks of n/k rows, the last one takes the remainder).  A shard may be empty (k < g). */
void rh_shard_chunks(uint64_t n, uint64_t num_chunks, uint32_t n_shards, uint32_t shard,
                     uint32_t* chunk_lo, uint32_t* chunk_hi, uint64_t* row_lo, uint64_t* row_hi);

typedef struct rh_stats rh_stats;

/* Call options.  Zero-initialise (memset / `rh_opts o = {0}`) and set `device = -1` for "current device"; fields
 * after `stream` were added in ABI version 3 and are all "0 = off". */
typedef struct {
  int32_t device;        /* HIP device ordinal; -1 = current device          */
  int32_t flags;         /* RH_KERNEL_* below; 0 = automatic                 */
  void* stream;          /* hipStream_t to launch on; NULL = engine's stream */
  /* Multi-GPU form of the chunk driver (rh_decode / rh_decode_packed): the reference deals its k chunks to a thread
   * pool (ruhvro/src/deserialize.rs:92-120); here the k chunks are dealt to `n_devices` shards in contiguous runs --
   * shard j decodes chunks [j*k/g, (j+1)*k/g) on HIP device devices[j], with its own host thread, streams and arenas
   * -- so every returned batch is produced entirely by one GPU and the result is identical for every g.  Ordinals may
   * repeat (several logical shards on one GPU).  NULL / 0 = the single device named by `device`. */
  const int32_t* devices;
  uint32_t n_devices;
  /* sizeof(rh_opts) as the caller compiled it, or 0.  0 = the ABI-3 layout, which ends with `device_stats`: the engine
   * then never reads the fields behind it, so a caller built against the shorter struct stays safe (the field was
   * `reserved0`, must-be-zero, in ABI 3).  Set it to sizeof(rh_opts) to use `ready` / `gathered`. */
  uint32_t struct_size;
  /* Explicit chunk geometry for a caller that decodes a RANGE of a larger call's chunks (one process per GPU, each
   * holding whole reference chunks): when non-zero, the n records are `num_chunks` chunks of `chunk_rows` rows, the
   * last one taking the rest (deserialize.rs:57-68 applied to the whole list, not to this range).  0 = the
   * reference's split of these n records (n / num_chunks). */
  uint64_t chunk_rows;
  rh_stats* device_stats; /* optional, room for n_devices entries: per-shard stage timings of a multi-GPU call */
  /* Streaming hand-over of the record slices (rh_decode only, ABI version 4): a producer thread of the caller fills
   * ptrs[] / lens[] front to back WHILE the call runs and publishes its progress in *ready -- the number of leading
   * entries that are valid (monotonic, stored with release order; UINT64_MAX = the producer gave up, the call fails
   * with RH_ERR_ARGUMENT).  The engine gathers a chunk group into pinned memory as soon as its entries are there, so
   * the H2D copy, the kernels and the D2H copy of the first groups overlap the producer's work on the later ones.
   * *gathered (optional) is the engine's answer: the number of leading records whose BYTES it has copied and will
   * not read again -- the caller may let go of them (the CPython boundary drops its references while the tail of the
   * call is still on the PCIe link).  NULL / NULL = every entry is valid at entry, the classic call.  Read only when
   * struct_size covers them. */
  const uint64_t* ready;
  uint64_t* gathered;
} rh_opts;

/* Kernel selection (rh_opts.flags).  Both forms are HIP kernels running the same field handlers and
 * produce identical buffers.  AUTO uses the kernels specialised to the schema when their code objects
 * are in the kernel cache, the generic schema-program interpreter otherwise -- and a call large enough
 * to be worth it (RUHVRO_HIP_SPECIALIZE_MIN records, default 32768) that misses the cache starts the
 * compile IN THE BACKGROUND (ABI version 6): that call and the ones after it run on the generic kernels
 * at once, the first call after the compile jobs finish switches over (rh_stats.specialized says which
 * form ran; rh_schema_kernels_ready waits for the switch).  A new schema therefore costs what it costs
 * the reference (src/lib.rs:39-54: a parse), not a compile.  RH_KERNEL_SPECIALIZED insists: the call
 * waits for the compile, or fails if there is no compiler. */
#define RH_KERNEL_AUTO 0
#define RH_KERNEL_GENERIC 1
#define RH_KERNEL_SPECIALIZED 2
/* rh_decode_device only (ABI version 4), OR-ed into rh_opts.flags: return as soon as the call is ON THE STREAM (size
 * pass, scan + arena layout, emit pass and the read-back of its control words all enqueued), without waiting for it.
 * The result's device buffers are valid in stream order on rh_opts.stream, like any asynchronous HIP work; what the
 * HOST learns from a call -- the first malformed record (the in-order join of deserialize.rs:115-119), row counts,
 * null counts, an arena that has to be re-laid-out -- is settled by rh_device_result_wait(), which every accessor of
 * an unsettled result also runs first.  Until then the input buffers (d_data, d_offsets) must stay alive AND UNMODIFIED,
 * and the compiled schema alive: the emit pass re-reads the records the size pass cleared and, in tiles without
 * anomalies, walks them with no bounds or anomaly predicate of its own (walk.h RH_TRUST) -- bytes that change between
 * the two passes (a caller recycling d_data on another stream) turn into unchecked stores.  Work that reuses the
 * buffers must be ordered behind the call on rh_opts.stream, or wait for rh_device_result_wait.  (RUHVRO_HIP_NO_TRUST=1
 * makes the emit pass walk every tile with its own checks -- a debugging aid, ~1.3x the kernel time.)  A schema's first call on a
 * device (no size history to reserve the arena from) completes synchronously whatever the flag says.  This is how a
 * pipeline of small batches keeps the GPU busy: a 1M-record call is 0.15 ms of kernels, and a synchronous call adds
 * ~25 us of host turn-around during which the GPU idles. */
#define RH_ASYNC 8
/* rh_decode_device only (ABI version 5), OR-ed into rh_opts.flags: the form of the launch sequence.
 * Default = two passes: a size pass (per-record sizes, tile totals), a scan + arena layout, an emit pass; every record is read
 * from HBM twice and 24 bytes of counters per record travel between the passes (4.8 GB per 10M benchmark records).
 * RH_SINGLE_PASS: prefer the single-pass form -- ONE kernel that sizes a tile, scans across the tiles of its chunk
 * (decoupled look-back, fence-free) and emits out of the same LDS window, into an arena laid out from per-column capacities
 * (the schema's size history): 3.0 GB per 10M records, 1.02 x the algorithmic bytes.  Needs the schema-specialised kernels
 * and a size history (a schema's first call is two-pass); a call that outgrows a capacity is repeated on the two-pass form
 * and the schema backs off.  Same buffers either way.  Measured on MI355X (profiles/r04v_*): about time-neutral at 10M
 * records (0.96-1.00 ms against 0.99-1.01), slower on small launches (the look-back wait is a fixed cost per tile) -- which
 * is why it is opt-in: its use is a deployment that is short of HBM bandwidth, not of time.  RUHVRO_HIP_SINGLE_PASS=1 makes it
 * the preference of every call; RH_TWO_PASS forces the two-pass form regardless. */
#define RH_TWO_PASS 16
#define RH_SINGLE_PASS 32

struct rh_stats {
  uint64_t records;
  uint64_t input_bytes;      /* Avro payload bytes                               */
  uint64_t output_bytes;     /* Arrow buffer bytes produced (all chunks)         */
  uint32_t chunks;
  uint32_t blocks;           /* workgroups per kernel launch                     */
  float pack_ms;             /* host gather of the record slices                 */
  float h2d_ms;
  float size_kernel_ms;      /* k_size   (walk 1: per-record sizes)              */
  float scan_kernel_ms;      /* k_scan   (segmented exclusive scans)             */
  float emit_kernel_ms;      /* k_emit   (walk 2: column materialisation)        */
  float d2h_ms;
  float total_ms;
  uint32_t specialized;      /* 1 = schema-specialised kernels ran, 0 = generic interpreter */
  uint32_t lds_bytes;        /* dynamic LDS per workgroup of the emit kernel                 */
};

/* Replaces ruhvro::deserialize::per_datum_deserialize_threaded
 * (ruhvro/src/deserialize.rs:76-121; single-chunk form per_datum_deserialize,
 * deserialize.rs:25-30, is num_chunks = 1).  Input: n record slices owned by
 * the caller for the duration of the call (src/lib.rs:29-33,84).  Output:
 * out_chunks[0..*out_k) are struct arrays (one per chunk, chunk boundaries of
 * deserialize.rs:57-68, order preserved) in host memory; the caller provides
 * room for rh_clamp_chunks(n, num_chunks) entries and releases each through
 * ArrowArray.release.  The first malformed record (lowest index) aborts the
 * call with its message, as the in-order join at deserialize.rs:115-119 does. */
int rh_decode(const rh_schema* s, const uint8_t* const* ptrs, const uint64_t* lens,
              uint64_t n, uint64_t num_chunks, const rh_opts* opts,
              struct ArrowArray* out_chunks, uint32_t* out_k, rh_stats* stats, char** err);

/* Same, for input already packed the way the reference packs it internally
 * (BinaryArray, deserialize.rs:90): one contiguous buffer + n+1 offsets. */
int rh_decode_packed(const rh_schema* s, const uint8_t* data, const uint64_t* offsets,
                     uint64_t n, uint64_t num_chunks, const rh_opts* opts,
                     struct ArrowArray* out_chunks, uint32_t* out_k, rh_stats* stats, char** err);

/* Device-resident form of the same path: `d_data`/`d_offsets` (u64[n+1]) live
 * in HBM (d_data 16-byte aligned, data_len = offsets[n]), the Arrow buffers are
 * produced in HBM and stay there.  This is the kernel-only path bench.py times.
 * The result owns its device memory. */
typedef struct rh_device_result rh_device_result;
int rh_decode_device(const rh_schema* s, const void* d_data, const void* d_offsets,
                     uint64_t data_len, uint64_t n, uint64_t num_chunks, const rh_opts* opts,
                     rh_device_result** out, rh_stats* stats, char** err);
/* Settle an RH_ASYNC call: waits for its stream, returns what the synchronous call would have returned (RH_OK, or
 * RH_ERR_DECODE with the reference's message for the lowest malformed record ...).  `stats` (optional) receives the
 * stage timings when the call was made with a non-NULL stats argument (which is itself not written by an asynchronous
 * call).  A no-op returning RH_OK on a result that is already settled.  Not thread-safe per result. */
int rh_device_result_wait(rh_device_result* r, rh_stats* stats, char** err);
uint32_t rh_device_result_chunks(const rh_device_result* r);
/* Exact (unpadded) Arrow buffer bytes the call produced, all chunks.  Settles an RH_ASYNC result first; 0 when that
 * call failed (rh_device_result_wait reports the message -- this accessor has no error channel). */
uint64_t rh_device_result_output_bytes(const rh_device_result* r);
/* Arrow C Device Data Interface view of chunk i (device_type ARROW_DEVICE_ROCM);
 * valid until rh_device_result_free; release the view through array.release. */
int rh_device_result_export(rh_device_result* r, uint32_t chunk, struct ArrowDeviceArray* out);
/* ABI version 6.  The device buffers of chunk i with their byte sizes (the Arrow C Device Data structs carry pointers and lengths
 * only): fills ptrs[] / sizes[] (either may be NULL) with up to `cap` entries, one per Arrow buffer of the schema, and returns how
 * many buffers a chunk has.  sizes[] are the bytes the engine reserved for the buffer (offsets: 4 x (rows + 1); bitmaps: whole
 * 64-bit words; data: the column's bytes), so a consumer can wrap buffers_of(export(i)) as typed device arrays without reading
 * an offsets buffer back -- what pyruhvro_amd.deserialize_to_device does for DLPack consumers.  0 on error. */
uint32_t rh_device_result_buffers(rh_device_result* r, uint32_t chunk, uint64_t* ptrs, uint64_t* sizes, uint32_t cap);
/* Copy the chunks to host memory (same form rh_decode returns). */
int rh_device_result_to_host(rh_device_result* r, struct ArrowArray* out_chunks, char** err);
void rh_device_result_free(rh_device_result* r);

/* Schema-specialised kernel management.  rh_schema_kernel_source returns the generated HIP source
 * (malloc'd, release with rh_free_string).  rh_schema_prebuild generates, compiles (hiprtc, gfx950;
 * needs no GPU) and stores the code objects (decode pair and encode pair) in the kernel cache so later
 * processes only load them; returns 0 and sets *cached = 1 when both were already there. */
char* rh_schema_kernel_source(const rh_schema* s);
/* Content hash (hex, malloc'd) of this schema's specialised decode (encode = 0) or encode (1) kernel pair: generated
 * source + every device header it includes.  It is the kernel-cache key; measurement files (profiles/hbm_traffic.json)
 * are stamped with it so that a number is only ever attributed to the kernel it was measured on. */
char* rh_schema_kernel_key(const rh_schema* s, int encode);
char* rh_schema_encode_kernel_source(const rh_schema* s);      /* the Arrow -> Avro pair (rh_encode) */
int rh_schema_prebuild(const rh_schema* s, int* cached, char** err);
/* ABI version 6.  State of the specialised decode (encode = 0) or encode (1) kernels of this schema: 1 = their code
 * objects are there (the next call runs on them), 0 = not yet (still compiling after timeout_ms, or nobody asked for them:
 * no call of RUHVRO_HIP_SPECIALIZE_MIN records yet and nothing in the kernel cache), -1 = the compile failed (*err).
 * Waits up to timeout_ms for running compile jobs (0 = just look, < 0 = no limit).  A service that wants its first batch
 * at full speed calls rh_schema_prebuild at start-up instead; this is for the ones that would rather start serving. */
int rh_schema_kernels_ready(const rh_schema* s, int encode, long timeout_ms, char** err);

/* The LEAN pair (added without a change of RH_ABI_VERSION: callers look these symbols up with dlsym).  rh_spec_size and
 * rh_spec_emit once more, compiled from the default source behind `#define RH_V_LEN16 1` and `#define RH_V_INT28 1` (walk.h):
 * lengths and block counts are read in the 2-byte form and ints in the 4-byte form.  A record that leaves those forms is
 * re-walked carefully and its tile flagged, so the pair is correct on any input; it is faster on batches of short varints
 * and slower on others, and the engine chooses per (schema, device): a qualifying call (AUTO or SPECIALIZED kernels, two-pass,
 * no ranged pair in the call, at least RUHVRO_HIP_LEAN_MIN_RECORDS records -- default 1,000,000, 0 = never) probes a sample
 * of its own tiles with the lean size kernel; a clean probe moves the schema to the lean pair, a lean call that meets a
 * careful tile or a re-walked wavefront moves it back for 8, 16, ... 1024 calls.  RUHVRO_HIP_LEAN=0 / 1: never / always.
 * A schema without a size pass and a wide schema have no lean pair.  rh_schema_kernel_source, rh_schema_kernel_key and
 * rh_schema_kernels_ready keep describing the default (wide) kernels, which the measurement stamps belong to.
 *   rh_schema_lean_kernel_source / _key   the lean source (malloc'd) and its kernel-cache key; NULL = no lean pair
 *   rh_schema_lean_ready                  like rh_schema_kernels_ready for the lean pair; -2 = the schema has none
 *   rh_schema_lean_state                  -1 no lean pair, 0 undecided, 1 lean, 2 wide -- of this schema on `device`
 *   rh_lean_counters                      fills out[0..n) with the RH_LEAN_* values below, returns RH_LEAN_COUNT */
char* rh_schema_lean_kernel_source(const rh_schema* s);
char* rh_schema_lean_kernel_key(const rh_schema* s);
int rh_schema_lean_ready(const rh_schema* s, long timeout_ms, char** err);
int rh_schema_lean_state(const rh_schema* s, int device);
enum {
  RH_LEAN_CALLS = 0,            /* decode calls that launched the lean pair                                                  */
  RH_LEAN_PROBES = 1,           /* probes settled (the lean size kernel over a sample of a call's tiles)                       */
  RH_LEAN_PROBES_CLEAN = 2,     /* ... without a careful tile, a re-walked wavefront or an error: the schema went lean         */
  RH_LEAN_PROBES_DIRTY = 3,     /* ... with one: the schema stays wide, the next probe comes 64 qualifying calls later         */
  RH_LEAN_FALLBACKS = 4,        /* lean calls whose own tile statistics moved the schema back to the wide pair                */
  RH_LEAN_RERUNS = 5,           /* lean calls repeated on another form by the settlement of an RH_ASYNC result                */
  RH_LEAN_NEED_RANGED = 6,      /* lean calls refused for a tile past the LDS window (repeated on the generic kernels)         */
  RH_LEAN_NEED_WIDE_INDEX = 7,  /* lean calls whose layout needs 64-bit indexing (repeated on the generic kernels)             */
  RH_LEAN_TWO_PASS_REPEATS = 8, /* two-pass repeats of a failed single-pass call that launched the lean pair                  */
  RH_LEAN_CAPACITY_TAILS = 9,   /* lean calls whose reserved arena was too small: tail re-run with the lean emit kernel        */
  RH_LEAN_ASYNC_SETTLED = 10,   /* lean calls made with RH_ASYNC and settled later                                             */
  RH_LEAN_COUNT = 11
};
uint32_t rh_lean_counters(uint64_t* out, uint32_t n);

/* Arrow -> Avro, the other direction.  Replaces ruhvro::serialize::serialize_record_batch
 * (ruhvro/src/serialize.rs:38-67) + fast_encode::serialize_chunk (ruhvro/src/fast_encode.rs:27-53): `batch` is
 * the record batch as a struct array (Arrow C Data Interface, any offsets / slices), columns are matched to the
 * schema's fields BY NAME (fast_encode.rs:151-185).  out_chunks[0..*out_k) are BinaryArrays ("z": i32 offsets +
 * data, one datum per row) in host memory, chunked like serialize.rs:19-30; the caller provides room for
 * rh_clamp_chunks(batch->length, num_chunks) entries and releases each through ArrowArray.release.  Data-dependent
 * failures return RH_ERR_DECODE with the reference's message text (fast_encode.rs:173-177, 541, 576). */
int rh_encode(const rh_schema* s, const struct ArrowArray* batch, const struct ArrowSchema* batch_schema,
              uint64_t num_chunks, const rh_opts* opts, struct ArrowArray* out_chunks, uint32_t* out_k,
              rh_stats* stats, char** err);

/* Device-resident form of rh_encode (the mirror of rh_decode_device): `batch` is a struct array whose BUFFER POINTERS
 * ARE DEVICE POINTERS on the call's device (what rh_device_result_export hands out: ArrowDeviceArray.array), read in
 * place -- no host copy.  Every buffer must be followed by at least 64 readable bytes (Arrow's own allocation padding;
 * the arenas of rh_decode_device are).  The k BinaryArrays ("z": i32 offsets + data, chunked like serialize.rs:19-30)
 * are produced in HBM and stay there: export chunk i as an ArrowDeviceArray (ARROW_DEVICE_ROCM), or copy all to the
 * host in the form rh_encode returns.  This is the kernel-only path `bench.py --direction encode` times. */
typedef struct rh_device_encoded rh_device_encoded;
int rh_encode_device(const rh_schema* s, const struct ArrowArray* batch, const struct ArrowSchema* batch_schema,
                     uint64_t num_chunks, const rh_opts* opts, rh_device_encoded** out, rh_stats* stats, char** err);
/* rh_encode with the result left in HBM (symbol added without a change of RH_ABI_VERSION): `batch` is a HOST batch, as
 * rh_encode's, and the BinaryArrays are an rh_device_encoded, as rh_encode_device's.  What rh_frame_join reads: the encoded
 * datums of a framed write cross PCIe once, as finished messages. */
int rh_encode_to_device(const rh_schema* s, const struct ArrowArray* batch, const struct ArrowSchema* batch_schema,
                        uint64_t num_chunks, const rh_opts* opts, rh_device_encoded** out, rh_stats* stats, char** err);
uint32_t rh_device_encoded_chunks(const rh_device_encoded* r);
uint64_t rh_device_encoded_output_bytes(const rh_device_encoded* r);   /* exact: i32 offsets + Avro bytes, all chunks */
int rh_device_encoded_export(rh_device_encoded* r, uint32_t chunk, struct ArrowDeviceArray* out);
int rh_device_encoded_to_host(rh_device_encoded* r, struct ArrowArray* out_chunks, char** err);
void rh_device_encoded_free(rh_device_encoded* r);

/* Process-wide counters of the engine's rarely taken branches (monotonic; tests read them before and after a call to
 * prove that the branch they aim at really ran).  Fills out[0..n) with as many of the RH_CTR_* values as fit; returns
 * RH_CTR_COUNT. */
enum {
  RH_CTR_FUSED_CALLS = 0,      /* decode calls that took the single-submission path (device-side arena layout)      */
  RH_CTR_TWO_SYNC_CALLS = 1,   /* ... that laid the arena out on the host between scan and emit (first call / env)  */
  RH_CTR_CAPACITY_RETRIES = 2, /* LF_CAPACITY: the arena reserved from the size history was too small, tail re-run  */
  RH_CTR_WIDE_FALLBACKS = 3,   /* NeedWideIndex: a call re-run on the generic kernels (64-bit in-buffer offsets)    */
  RH_CTR_OFFSET32_ERRORS = 4,  /* calls refused because a chunk's column exceeds 32-bit Arrow offsets               */
  RH_CTR_SPLIT_CALLS = 5,      /* device-resident calls that dealt their chunk groups to internal streams (in-call overlap) */
  RH_CTR_SINGLE_PASS_CALLS = 6, /* decode calls that took the single-pass form (one kernel sizes, scans across tiles and emits) */
  RH_CTR_SINGLE_PASS_FAILOVERS = 7, /* ... of which outgrew a column capacity and were repeated on the two-pass form */
  RH_CTR_BACKGROUND_COMPILES = 8, /* kernel compile jobs started behind a call that went ahead on the generic kernels (ABI 6) */
  /* ABI 7: what the walks met, summed over the tiles of every single-submission call on the device (the scan launch sums the
   * size pass's per-tile flags, the call's last kernel hands the sums over; a call's first run on a schema, a call repeated with an
   * exact arena and an attempt refused for want of the ranged kernels are not counted).  A call without a size pass (a schema
   * without variable-length output) counts only its tiles past the window -- over_window_tiles, subtiled_tiles -- in its emit
   * kernels, on every path.  A tile
   * is one workgroup's records (256, or 64 for wide schemas); all of these are 0 on input that stays inside the fast wire forms. */
  RH_CTR_TILES = 9,             /* tiles of the calls counted below                                                           */
  RH_CTR_CAREFUL_TILES = 10,    /* tiles the emit pass walked with the careful form (an anomaly in the size pass, or no window)  */
  RH_CTR_OVER_WINDOW_TILES = 11, /* tiles whose bytes did not fit the LDS window in one piece                                  */
  RH_CTR_REWALKED_WAVES = 12,   /* wavefronts the size pass walked twice (a record outside the fast wire forms, or malformed)  */
  RH_CTR_SUBTILED_TILES = 13,   /* over-window tiles that were staged through the window in record ranges (not walked from HBM) */
  RH_CTR_RANGED_RETRIES = 14,   /* calls repeated on the generic kernels: a tile past the window met specialised kernels whose ranged pair was not loaded yet */
  /* Tolerant decode (rh_decode*_tolerant below; appended without a change of RH_ABI_VERSION) */
  RH_CTR_TOLERANT_CALLS = 15,   /* tolerant decode calls                                                                      */
  RH_CTR_TOLERANT_REPAIRS = 16, /* ... of which met a malformed record: they ran the validation kernel and a second decode    */
  RH_CTR_COUNT = 17
};
uint32_t rh_engine_counters(uint64_t* out, uint32_t n);

/* Tolerant decode.  A strict decode call (rh_decode / rh_decode_packed / rh_decode_device) is aborted by its lowest malformed
 * record, as the reference's is.  A tolerant call returns the batches of the strict call -- same number of chunks, same chunk
 * boundaries, same rows -- in which every malformed record has been REPLACED by the schema's placeholder datum, and the list of
 * ALL malformed records as (index, message), ascending by index; `message` is exactly what the strict call raises when that
 * record is the lowest failing one.  In other words: the batches are, buffer for buffer, those of the strict call on the input
 * with the placeholder in place of every listed record.
 * The placeholder is the shortest datum of the schema the strict decoder accepts (null wherever the schema allows null, zero /
 * empty elsewhere): null -> nothing; boolean, int, long and their logical types, enum, string, bytes, array, map -> 00; float /
 * double -> 4 / 8 zero bytes; uuid on string -> the 36-character nil uuid behind its length; decimal on bytes -> 02 00;
 * fixed(n) and decimal / duration / uuid over it -> n zero bytes; record -> its fields' placeholders; a union with a null branch
 * -> the index of its first null branch; any other union -> branch 0 and that branch's placeholder.
 * The call is optimistic: it IS the strict call, and a clean input costs exactly what the strict call costs (no extra launch,
 * allocation or copy).  Only when the strict call fails on a record, a validation kernel walks all n records, the malformed
 * ones are replaced and the strict call runs again on the patched input (the device form gathers it into a new device buffer
 * that the result owns).  More than `max_errors` malformed records (1024 is a sensible bound: beyond it the schema is wrong,
 * not the data) fail the call with the strict call's error; max_errors = 0 is the strict call.  Errors that belong to no single
 * record (offset overflow, runtime failures) are returned as by the strict call.  Projected schemas compose: the errors are the
 * full decode's, the placeholder the full schema's.  RH_ASYNC is refused with RH_ERR_ARGUMENT; every other flag and field of
 * rh_opts means what it means for the strict call.
 * Added WITHOUT a change of RH_ABI_VERSION (7): a caller discovers these entry points by the presence of the symbols (dlsym). */
/* The placeholder datum: *bytes (owned by the schema, valid until rh_schema_free) and *len. */
int rh_schema_placeholder(const rh_schema* s, const uint8_t** bytes, uint64_t* len);
/* The list of malformed records a call reports: opaque, released with rh_record_errors_free.  rh_record_errors_get: entry i
 * (ascending record index) -> its record index, its error code and its message (owned by the list); any out pointer may be NULL. */
typedef struct rh_record_errors rh_record_errors;
uint64_t rh_record_errors_count(const rh_record_errors* e);
int rh_record_errors_get(const rh_record_errors* e, uint64_t i, uint64_t* index, int* code, const char** message);
void rh_record_errors_free(rh_record_errors* e);
/* Validation alone: *out lists ALL malformed records of the input -- when there are more than max_errors, the max_errors
 * lowest -- and *total_bad is their exact number.  Host input is uploaded in groups and validated on rh_opts.device (the first
 * entry of rh_opts.devices for a multi-device option block). */
int rh_validate(const rh_schema* s, const uint8_t* const* ptrs, const uint64_t* lens, uint64_t n, const rh_opts* opts,
                uint64_t max_errors, rh_record_errors** out, uint64_t* total_bad, char** err);
int rh_validate_packed(const rh_schema* s, const uint8_t* data, const uint64_t* offsets, uint64_t n, const rh_opts* opts,
                       uint64_t max_errors, rh_record_errors** out, uint64_t* total_bad, char** err);
int rh_validate_device(const rh_schema* s, const void* d_data, const void* d_offsets, uint64_t data_len, uint64_t n,
                       const rh_opts* opts, uint64_t max_errors, rh_record_errors** out, uint64_t* total_bad, char** err);
/* The tolerant forms of rh_decode, rh_decode_packed and rh_decode_device: their arguments, then max_errors and the list
 * (*errors: empty for a clean input, NULL when the call fails). */
int rh_decode_tolerant(const rh_schema* s, const uint8_t* const* ptrs, const uint64_t* lens, uint64_t n, uint64_t num_chunks,
                       const rh_opts* opts, struct ArrowArray* out_chunks, uint32_t* out_k, rh_stats* stats, char** err,
                       uint64_t max_errors, rh_record_errors** errors);
int rh_decode_packed_tolerant(const rh_schema* s, const uint8_t* data, const uint64_t* offsets, uint64_t n, uint64_t num_chunks,
                              const rh_opts* opts, struct ArrowArray* out_chunks, uint32_t* out_k, rh_stats* stats, char** err,
                              uint64_t max_errors, rh_record_errors** errors);
int rh_decode_device_tolerant(const rh_schema* s, const void* d_data, const void* d_offsets, uint64_t data_len, uint64_t n,
                              uint64_t num_chunks, const rh_opts* opts, rh_device_result** out, rh_stats* stats, char** err,
                              uint64_t max_errors, rh_record_errors** errors);

/* Avro object container files.  Added WITHOUT a change of RH_ABI_VERSION (7): a caller discovers these entry
 * points by the presence of the symbols (dlsym).
 *
 * rh_container_scan parses the framing of a container held in host memory -- the header (magic, metadata map, sync marker) and
 * the chain of blocks -- without touching a device: every read is checked against `len`.  It fails with RH_ERR_DECODE and a
 * message that starts with "container: " (naming the block index where there is one) for a bad magic, a truncated header, a
 * header without avro.schema, a negative count or size, a size past the end of the file, a sync marker that does not match,
 * bytes left after the last complete block, and a codec other than "null" / "deflate".  The accessors' pointers belong to the
 * info object (rh_container_info_free).  The block table: the payload of block b is bytes [start[b], end[b]) of the file and
 * its first record has index first[b]; first[nb] = n.  A block without records and a file without blocks are legal.
 * rh_container_info_metadata_*: the header's entries other than avro.schema and avro.codec, in file order. */
typedef struct rh_container_info rh_container_info;
int rh_container_scan(const uint8_t* data, uint64_t len, rh_container_info** info, char** err);
const char* rh_container_info_schema(const rh_container_info* i, uint64_t* len);
const char* rh_container_info_codec(const rh_container_info* i);       /* "null" when the header names none */
const uint8_t* rh_container_info_sync(const rh_container_info* i);     /* 16 bytes */
uint64_t rh_container_info_blocks(const rh_container_info* i);
uint64_t rh_container_info_records(const rh_container_info* i);
int rh_container_info_table(const rh_container_info* i, const uint64_t** start, const uint64_t** end, const uint64_t** first);
uint32_t rh_container_info_metadata_count(const rh_container_info* i);
int rh_container_info_metadata_get(const rh_container_info* i, uint32_t k, const char** key, const uint8_t** value, uint64_t* value_len);
void rh_container_info_free(rh_container_info* i);
/* The blocks call: `data` (host memory, `len` bytes) holds UNCOMPRESSED block payloads at [start[b], end[b]) -- a "null"-codec
 * file as it is with the table of rh_container_scan, or a caller's own buffer of inflated blocks (ascending, not overlapping;
 * the C ABI has no codec of its own).  The buffer and the table are uploaded once; a split kernel (one lane per block) walks
 * every block's records with the WRITER's schema and leaves their offsets on the device; the device-input decode of
 * rh_decode_device then runs on them.  The batches are those of rh_decode over the same records: same chunk rule, any kernel
 * mode, `s` plain, projected (rh_schema_project) or resolved (rh_schema_resolve) -- the split always walks the plain schema
 * such an `s` was made from.  A malformed record fails the call with rh_decode's message for the lowest failing record
 * (RH_ERR_DECODE); a block whose records do not end where the block does fails it with "container: block b: its N records end
 * at byte X of Y"; a block of 4 GiB - 16 bytes or more, or one whose count cannot fit its size, is refused likewise.  One
 * device: rh_opts.devices (multi-device), RH_ASYNC and chunk_rows are refused with RH_ERR_ARGUMENT.  n = 0 gives one empty batch.
 * rh_decode_blocks exports to host memory as rh_decode_packed does; rh_decode_blocks_device leaves the buffers in HBM (the
 * result owns the uploaded bytes too).  rh_split_last_ms: GPU time of the most recent call's split kernel in this process. */
int rh_decode_blocks(const rh_schema* s, const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end,
                     const uint64_t* first, uint64_t nb, uint64_t num_chunks, const rh_opts* opts, struct ArrowArray* out_chunks,
                     uint32_t* out_k, rh_stats* stats, char** err);
int rh_decode_blocks_device(const rh_schema* s, const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end,
                            const uint64_t* first, uint64_t nb, uint64_t num_chunks, const rh_opts* opts, rh_device_result** out,
                            rh_stats* stats, char** err);
float rh_split_last_ms(void);

/* Deflate blocks inflated on the device ("Deflate blocks on the device").  Added WITHOUT a change of
 * RH_ABI_VERSION (7), like the entry points above: a caller discovers them by the presence of the symbols (dlsym).
 *
 * rh_decode_cblocks / rh_decode_cblocks_device are rh_decode_blocks / rh_decode_blocks_device with a codec: for
 * RH_CODEC_DEFLATE `start` / `end` delimit the COMPRESSED payloads -- raw deflate (RFC 1951), one stream per block, the table
 * of rh_container_scan as it is.  The file is uploaded compressed; a size kernel walks every stream (one wavefront per block)
 * and reports its inflated size and its verdict, the host lays the blocks out back to back, an emit kernel writes their bytes,
 * and the call goes on as rh_decode_blocks does from its upload.  What is a valid stream is what zlib's inflate accepts.  A
 * block that does not inflate fails the call with RH_ERR_DECODE before any record is walked, the lowest such block first:
 * "container: block b: deflate: <reason>" for a malformed stream (the reasons: DESIGN.md 14), "... deflate: the stream ends
 * before its final block", "... deflate: N bytes behind the end of the stream", "... deflate: it inflates to L bytes or more
 * (a block of 4 GiB - 16 bytes or more is not supported)" with L = max_block_bytes (0: the engine's own limit, 4 GiB - 16).  The
 * checks of rh_decode_blocks on a block's size and record count apply to the INFLATED sizes.  The refusals are those of
 * rh_decode_blocks (devices, RH_ASYNC, chunk_rows); codec = RH_CODEC_NULL is rh_decode_blocks (max_block_bytes is not read). */
#define RH_CODEC_NULL 0
#define RH_CODEC_DEFLATE 1
int rh_decode_cblocks(const rh_schema* s, const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end,
                      const uint64_t* first, uint64_t nb, int codec, uint64_t max_block_bytes, uint64_t num_chunks, const rh_opts* opts,
                      struct ArrowArray* out_chunks, uint32_t* out_k, rh_stats* stats, char** err);
int rh_decode_cblocks_device(const rh_schema* s, const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end,
                             const uint64_t* first, uint64_t nb, int codec, uint64_t max_block_bytes, uint64_t num_chunks,
                             const rh_opts* opts, rh_device_result** out, rh_stats* stats, char** err);
/* The inflate step alone, host in and host out: the nb streams at data[start[b] .. end[b]) inflated by the same two kernels.
 * Returns RH_OK with one status PER BLOCK -- one launch gives the verdicts of thousands of damaged streams.  *out (malloc'd,
 * release with rh_free_string) holds the accepted blocks back to back, block b at [out_start[b], out_end[b]); a failing block
 * contributes zero bytes.  reason: which rule a malformed stream broke (RH_INFLATE_MALFORMED only; pyruhvro_amd/csrc/
 * inflate_core.h R_*).  detail: RH_INFLATE_TRAILING -- the whole bytes behind the byte that holds the stream's
 * last bit (zlib's unused_data); RH_INFLATE_TOO_LARGE -- the limit; RH_INFLATE_MALFORMED -- which code, for the rules about a
 * code (0 code-length, 1 literal/length, 2 distance).  RH_INFLATE_INTERNAL is never returned: it fails the call. */
#define RH_INFLATE_OK 0
#define RH_INFLATE_MALFORMED 1
#define RH_INFLATE_TRUNCATED 2
#define RH_INFLATE_TRAILING 3
#define RH_INFLATE_TOO_LARGE 4
#define RH_INFLATE_INTERNAL 5
typedef struct rh_inflate_status {
  uint32_t code;
  uint32_t reason;
  uint64_t detail;
} rh_inflate_status;
int rh_inflate_blocks(const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end, uint64_t nb, uint64_t max_block_bytes,
                      const rh_opts* opts, uint8_t** out, uint64_t* out_len, uint64_t* out_start, uint64_t* out_end,
                      rh_inflate_status* status, char** err);
/* The most recent device inflate of this process: GPU time of its two kernels, compressed bytes in, inflated bytes out. */
void rh_inflate_last(float* size_ms, float* emit_ms, uint64_t* in_bytes, uint64_t* out_bytes);

/* Deflate blocks written on the device.  Added WITHOUT a change of RH_ABI_VERSION (7), discovered by symbol.
 *
 * rh_deflate_blocks is the twin of rh_inflate_blocks, host in and host out: the nb payloads at data[start[b] .. end[b]) each
 * become one raw RFC 1951 stream, compressed by rh_k_deflate in segments of 32 KiB (one wavefront each) and gathered back to
 * back by rh_k_deflate_gather.  *out (malloc'd, release with rh_free_string) holds the streams, stream b at
 * [out_start[b], out_end[b]); every stream is at most rh_deflate_bound(end[b] - start[b]) bytes.  strategy: which block forms
 * the writer may choose from -- a segment that would not fit its slot in the form asked for is written stored all the same.
 * The table is checked as rh_inflate_blocks checks it, before any device work; a payload of 4 GiB - 16 bytes or more is refused
 * ("container: block b: a block of 4 GiB - 16 bytes or more is not supported (N bytes)"); rh_opts.devices and RH_ASYNC are
 * refused.  rh_deflate_blocks_host runs the same stream logic (pyruhvro_amd/csrc/deflate_core.h) on the calling thread, with no
 * device: its bytes are the device's bytes. */
#define RH_DEFLATE_AUTO 0
#define RH_DEFLATE_STORED 1
#define RH_DEFLATE_FIXED 2
#define RH_DEFLATE_DYNAMIC 3
int rh_deflate_blocks(const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end, uint64_t nb, uint32_t strategy,
                      const rh_opts* opts, uint8_t** out, uint64_t* out_len, uint64_t* out_start, uint64_t* out_end, char** err);
int rh_deflate_blocks_host(const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end, uint64_t nb, uint32_t strategy,
                           uint8_t** out, uint64_t* out_len, uint64_t* out_start, uint64_t* out_end, char** err);
/* The largest size a stream for len bytes can take: len + 10 * max(1, ceil(len / 32768)) - 5. */
uint64_t rh_deflate_bound(uint64_t len);
/* The most recent device deflate of this process: GPU time of its two kernels, payload bytes in, stream bytes out. */
void rh_deflate_last(float* deflate_ms, float* gather_ms, uint64_t* in_bytes, uint64_t* out_bytes);

/* Tolerant container reads.  Added WITHOUT a change of RH_ABI_VERSION (7), discovered by symbol.
 *
 * rh_container_salvage is rh_container_scan that goes on past a block it cannot frame: it searches for the next occurrence of
 * the file's sync marker and frames again behind it.  It fails only where the HEADER does not parse (the messages of
 * rh_container_scan).  The info object's table (rh_container_info_table) lists the framed blocks; rh_container_info_salvage adds,
 * per block, the offset of its header and the count its header claims, and `refused` = 1 where that count is one the running
 * total cannot take ("record count out of range": it counts as 0 in `first`).  A gap is a stretch of bytes in which no block
 * was framed: [offset, offset + length), `block` = the blocks framed in front of it, `message` = what rh_container_scan says
 * at `offset`.  Blocks and gaps tile [header_end, len) exactly.  On a file rh_container_scan accepts the table is the same and
 * there are no gaps.  `steps`: loop turns of the scan (linear in len whatever the bytes are). */
int rh_container_salvage(const uint8_t* data, uint64_t len, rh_container_info** info, char** err);
int rh_container_info_salvage(const rh_container_info* i, uint64_t* header_end, const uint64_t** header_offset, const uint64_t** count,
                              const uint8_t** refused, uint64_t* gaps, uint64_t* steps);
int rh_container_info_gap(const rh_container_info* i, uint64_t k, uint64_t* offset, uint64_t* length, uint64_t* block, const char** message);
/* What became of one block of a tolerant blocks call.  code: 0 = sound (kept = its count); an ErrCode (1 .. 0xFF) = record `kept`
 * is malformed, detail as rh_validate's; RH_BLOCK_END = its records end at byte `detail` of its `aux` bytes (kept = its count);
 * RH_BLOCK_DROPPED = the caller passed it in as dropped; RH_BLOCK_COUNT / RH_BLOCK_TOO_LARGE = its count / size is refused,
 * detail = its (inflated) size; RH_BLOCK_INFLATE + an RH_INFLATE_* code = its deflate stream is refused, aux and detail the
 * rh_inflate_status's reason and detail.  rh_block_status_message: the message the strict call raises for that block (`count` =
 * what its header claims); release with rh_free_string. */
#define RH_BLOCK_END 0x100
#define RH_BLOCK_DROPPED 0x200
#define RH_BLOCK_COUNT 0x201
#define RH_BLOCK_TOO_LARGE 0x202
#define RH_BLOCK_INFLATE 0x300
typedef struct rh_block_status {
  uint32_t code;
  uint32_t aux;
  int64_t detail;
  uint64_t kept;
} rh_block_status;
int rh_block_status_message(uint64_t block, const rh_block_status* status, uint64_t count, char** message);
/* rh_decode_cblocks / rh_decode_cblocks_device in the tolerant form: a block that fails costs the call that block's failing
 * records, not the call.  A block with dropped[b] != 0 (dropped may be NULL), a block whose count or size the strict call
 * refuses and a block whose deflate stream is refused are not walked and keep nothing; rh_k_split_salvage walks the others,
 * every lane stopping its own block at its first malformed record; what is kept is gathered into one buffer
 * (rh_k_salvage_gather) and decoded as rh_decode_device decodes it -- the batches are those of the kept records, in file order,
 * chunked by num_chunks.  status[nb] says what became of every block.  A call in which nothing is reported launches no gather.
 * More than max_errors reports -- the blocks with a non-zero code plus extra_errors, the caller's own (gaps) -- set *too_many
 * = 1 and return RH_OK with no result: the caller runs the strict call for its error.  Failures that belong to no block fail
 * the call as they fail the strict one, and so do its refusals (devices, RH_ASYNC, chunk_rows).  rh_decode_blocks_tolerant
 * writes at most out_cap chunks (rh_clamp_chunks(first[nb], num_chunks) always suffices). */
int rh_decode_blocks_tolerant(const rh_schema* s, const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end,
                              const uint64_t* first, const uint8_t* dropped, uint64_t nb, int codec, uint64_t max_block_bytes,
                              uint64_t max_errors, uint64_t extra_errors, uint64_t num_chunks, const rh_opts* opts,
                              struct ArrowArray* out_chunks, uint32_t out_cap, uint32_t* out_k, rh_block_status* status, int* too_many,
                              rh_stats* stats, char** err);
int rh_decode_blocks_tolerant_device(const rh_schema* s, const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end,
                                     const uint64_t* first, const uint8_t* dropped, uint64_t nb, int codec, uint64_t max_block_bytes,
                                     uint64_t max_errors, uint64_t extra_errors, uint64_t num_chunks, const rh_opts* opts,
                                     rh_device_result** out, rh_block_status* status, int* too_many, rh_stats* stats, char** err);
/* The most recent tolerant blocks call of this process: GPU time of its split and of its gather (0 = none ran), the blocks it
 * reported (extra_errors not among them), the bytes it gathered (0 = the buffer was decoded where it was). */
void rh_salvage_last(float* split_ms, float* gather_ms, uint64_t* blocks_reported, uint64_t* bytes_gathered);

/* Row filters.  Added WITHOUT a change of RH_ABI_VERSION (7), discovered by symbol.
 *
 * A filtered strict decode returns, buffer for buffer, the strict decode of the records whose values match a predicate -- the
 * records are chosen on the device, from the raw bytes, before anything is decoded.  A predicate is 1 to 8 terms, ANDed; a term
 * names a top-level field of the WRITER schema (whether or not the call's projection or reader schema builds it), an operator
 * ("==" "!=" "<" "<=" ">" ">=" "is_null" "not_null") and a value.  Fields: int / long and their logical types (int64 order),
 * float / double (the value widened to double, IEEE order: NaN fails everything but "!=", -0.0 == 0.0), boolean and enum ("==" /
 * "!=" only; an enum against one of its symbol names), string / bytes (unsigned bytewise order, a proper prefix first, at most
 * 255 comparand bytes); plain or in a union with null, either order.  A null value fails every comparison, "!=" included; on a
 * field that cannot be null "is_null" keeps nothing and "not_null" everything.
 * rh_filter_compile refuses, with RH_ERR_SCHEMA and a message that starts with "where: " and names the field: an unknown field or
 * a dotted path, a field of any other kind ("not supported yet"), an operator the kind does not take, a value of the wrong kind or
 * out of range, an unknown enum symbol, a comparand over 255 bytes, zero terms or more than 8.  `writer` is a schema of
 * rh_schema_compile: a projected or resolved one is RH_ERR_ARGUMENT.  The filter is immutable and does not reference `writer`.
 * Every record is walked in full with the strict decode's checks: a malformed record fails the call with the strict decode's
 * message for the lowest failing record of the WHOLE list (RH_ERR_DECODE), whatever the predicate says about it.
 * rh_filter_packed / rh_filter_device: the kernel alone -- bit i of keep_words[i / 64] (room for ceil(n / 64) words, host memory)
 * says whether record i is kept, *kept how many are.
 * rh_decode_where / rh_decode_packed_where / rh_decode_device_where: rh_decode / rh_decode_packed / rh_decode_device with the
 * filter -- `s` plain, projected or resolved, made from the writer schema the filter was compiled against (else
 * RH_ERR_ARGUMENT).  num_chunks applies to the kept records (out_chunks: room for rh_clamp_chunks(n, num_chunks) always suffices);
 * nothing kept gives what a decode of no records gives.  A call that keeps every record decodes its input where it is; otherwise
 * the kept records are gathered into a device buffer the result owns.  The host forms upload the list in one piece (not the
 * pinned, pipelined path of rh_decode).  One device: rh_opts.devices and RH_ASYNC are refused with RH_ERR_ARGUMENT.
 * rh_filter_last: GPU time of the most recent call's filter kernel and of its compaction (offsets + gather; 0 = none ran), the
 * records it was given and the records it kept. */
typedef struct rh_filter rh_filter;
#define RH_FILTER_VALUE_NONE 0     /* is_null / not_null                                                       */
#define RH_FILTER_VALUE_INT 1      /* i, and the same value in d                                               */
#define RH_FILTER_VALUE_DOUBLE 2   /* d                                                                        */
#define RH_FILTER_VALUE_BOOL 3     /* i = 0 / 1                                                                */
#define RH_FILTER_VALUE_BYTES 4    /* bytes[0 .. len): UTF-8 text or raw bytes, an enum symbol's name           */
#define RH_FILTER_VALUE_BIGINT 5   /* an integer outside the int64 range: d holds it (refused for int / long)   */
typedef struct rh_filter_term {
  const char* name;
  const char* op;
  int32_t value_kind;
  int32_t reserved;
  int64_t i;
  double d;
  const uint8_t* bytes;
  uint64_t len;
} rh_filter_term;
int rh_filter_compile(const rh_schema* writer, const rh_filter_term* terms, uint32_t n, rh_filter** out, char** err);
void rh_filter_free(rh_filter* f);
int rh_filter_packed(const rh_filter* f, const uint8_t* data, const uint64_t* offsets, uint64_t n, const rh_opts* opts,
                     uint64_t* keep_words, uint64_t* kept, char** err);
int rh_filter_device(const rh_filter* f, const void* d_data, const void* d_offsets, uint64_t data_len, uint64_t n, const rh_opts* opts,
                     uint64_t* keep_words, uint64_t* kept, char** err);
int rh_decode_where(const rh_schema* s, const uint8_t* const* ptrs, const uint64_t* lens, uint64_t n, uint64_t num_chunks,
                    const rh_opts* opts, struct ArrowArray* out_chunks, uint32_t* out_k, rh_stats* stats, char** err,
                    const rh_filter* filter, uint64_t* kept);
int rh_decode_packed_where(const rh_schema* s, const uint8_t* data, const uint64_t* offsets, uint64_t n, uint64_t num_chunks,
                           const rh_opts* opts, struct ArrowArray* out_chunks, uint32_t* out_k, rh_stats* stats, char** err,
                           const rh_filter* filter, uint64_t* kept);
int rh_decode_device_where(const rh_schema* s, const void* d_data, const void* d_offsets, uint64_t data_len, uint64_t n,
                           uint64_t num_chunks, const rh_opts* opts, rh_device_result** out, rh_stats* stats, char** err,
                           const rh_filter* filter, uint64_t* kept);
void rh_filter_last(float* filter_ms, float* gather_ms, uint64_t* n, uint64_t* kept);

/* Row filters in the container read.  Added WITHOUT a change of RH_ABI_VERSION (7), discovered by symbol.
 *
 * rh_decode_blocks_where / rh_decode_blocks_device_where / rh_decode_cblocks_where / rh_decode_cblocks_device_where: their strict
 * twins with a predicate of rh_filter_compile.  The split kernel's walk -- the one careful walk of every record a container read
 * makes anyway -- also evaluates the predicate; the batches are those of rh_decode over the records it keeps, in file order
 * (num_chunks applies to them; nothing kept gives what a decode of no records gives).  A call that keeps every record decodes
 * the uploaded buffer where it is; otherwise the kept records are gathered into a device buffer the result owns.  `s` is plain,
 * projected or resolved, made from the writer text the filter was compiled against (else RH_ERR_ARGUMENT).  They refuse what the
 * blocks calls refuse (devices, RH_ASYNC, chunk_rows, the table, a block's size and count), with the same messages, and a
 * malformed record or block fails the call exactly as it fails the strict twin, whether or not the record would have matched.
 * rh_filter_blocks / rh_filter_cblocks: the split and the predicate alone -- bit i of keep_words[i / 64] (host memory, room for
 * ceil(first[nb] / 64) words) says whether record i of the file is kept, *kept how many are.
 * rh_container_where_last: GPU time of the most recent such call's split kernel and of its compaction (offsets + gather; 0 = none
 * ran: every record was kept, or the call was rh_filter_*blocks), the records of the file and the records kept. */
int rh_decode_blocks_where(const rh_schema* s, const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end,
                           const uint64_t* first, uint64_t nb, uint64_t num_chunks, const rh_opts* opts, struct ArrowArray* out_chunks,
                           uint32_t* out_k, rh_stats* stats, char** err, const rh_filter* filter, uint64_t* kept);
int rh_decode_blocks_device_where(const rh_schema* s, const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end,
                                  const uint64_t* first, uint64_t nb, uint64_t num_chunks, const rh_opts* opts, rh_device_result** out,
                                  rh_stats* stats, char** err, const rh_filter* filter, uint64_t* kept);
int rh_decode_cblocks_where(const rh_schema* s, const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end,
                            const uint64_t* first, uint64_t nb, int codec, uint64_t max_block_bytes, uint64_t num_chunks, const rh_opts* opts,
                            struct ArrowArray* out_chunks, uint32_t* out_k, rh_stats* stats, char** err, const rh_filter* filter,
                            uint64_t* kept);
int rh_decode_cblocks_device_where(const rh_schema* s, const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end,
                                   const uint64_t* first, uint64_t nb, int codec, uint64_t max_block_bytes, uint64_t num_chunks,
                                   const rh_opts* opts, rh_device_result** out, rh_stats* stats, char** err, const rh_filter* filter,
                                   uint64_t* kept);
int rh_filter_blocks(const rh_filter* f, const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end, const uint64_t* first,
                     uint64_t nb, const rh_opts* opts, uint64_t* keep_words, uint64_t* kept, char** err);
int rh_filter_cblocks(const rh_filter* f, const uint8_t* data, uint64_t len, const uint64_t* start, const uint64_t* end, const uint64_t* first,
                      uint64_t nb, int codec, uint64_t max_block_bytes, const rh_opts* opts, uint64_t* keep_words, uint64_t* kept, char** err);
void rh_container_where_last(float* split_ms, float* gather_ms, uint64_t* n, uint64_t* kept);

/* Framed messages.  Added WITHOUT a change of RH_ABI_VERSION (7), discovered by symbol.
 *
 * Messages as a Kafka consumer holds them -- a header in front of every datum -- are checked, partitioned by writer schema id and
 * stripped of their headers on the device; each class is then decoded by the unchanged strict decode with its own schema.
 *   RH_FRAMING_CONFLUENT      00 | schema id, 4 bytes big-endian | datum                       (ids 0 .. 2^32 - 1)
 *   RH_FRAMING_SINGLE_OBJECT  C3 01 | CRC-64-AVRO fingerprint, 8 bytes little-endian | datum  (ids 0 .. 2^64 - 1)
 * rh_frame_split_packed / rh_frame_split_device: `ids` are the m (1 .. 32) wire ids of the call, ascending and distinct; class c is
 * the messages whose header carries ids[c], in input order.  Framing is judged over the whole list before anything else happens:
 * the message of the lowest index that is shorter than the header, does not start with the marker, or -- without
 * RH_FRAME_SKIP_UNKNOWN -- carries an id that is not in `ids` fails the call with RH_ERR_DECODE and a message that starts with
 * "framed: message <i> ".  With RH_FRAME_SKIP_UNKNOWN the messages of unknown ids form class m: they have indices and no payload.
 * RH_FRAME_CLASSIFY_ONLY (implies the former): the verdicts alone, no partition.  The host form uploads the list in one piece (not
 * the pinned, pipelined path of rh_decode); the device form takes rh_decode_device's input (payload 16-byte aligned).  One device:
 * rh_opts.devices and RH_ASYNC are refused with RH_ERR_ARGUMENT.  The split owns device memory until rh_frame_split_free.
 * rh_frame_split_count: messages of class c (c = m: the unknown ids).  rh_frame_split_classes: one byte per message -- its class,
 * or 0xFD for an unknown id -- into n bytes of host memory.  rh_frame_split_indices: class c's ascending positions in the input,
 * into rh_frame_split_count(c) int64 of host memory.
 * rh_frame_decode_class: rh_decode_packed of class c's payloads with `s` -- plain, projected or resolved, made from that class's
 * writer schema; num_chunks applies to the class (out_chunks: room for rh_clamp_chunks(rh_frame_split_count(c), num_chunks)).  A
 * malformed payload raises "framed: schema id <id>: " and the strict decode's message for the class's list.  The result takes the
 * class's payloads over: a class decodes once.
 * rh_frame_last: GPU time of the most recent split's classify kernel, of its scan and offsets kernels, and of its gather. */
typedef struct rh_frame_split rh_frame_split;
#define RH_FRAMING_CONFLUENT 0
#define RH_FRAMING_SINGLE_OBJECT 1
#define RH_FRAME_SKIP_UNKNOWN 1
#define RH_FRAME_CLASSIFY_ONLY 2
int rh_frame_split_packed(const uint8_t* data, const uint64_t* offsets, uint64_t n, const uint64_t* ids, uint32_t m, uint32_t framing,
                          uint32_t flags, const rh_opts* opts, rh_frame_split** out, char** err);
int rh_frame_split_device(const void* d_data, const void* d_offsets, uint64_t data_len, uint64_t n, const uint64_t* ids, uint32_t m,
                          uint32_t framing, uint32_t flags, const rh_opts* opts, rh_frame_split** out, char** err);
uint64_t rh_frame_split_count(const rh_frame_split* split, uint32_t c);
int rh_frame_split_classes(const rh_frame_split* split, uint8_t* out, char** err);
int rh_frame_split_indices(const rh_frame_split* split, uint32_t c, int64_t* out, char** err);
int rh_frame_decode_class(rh_frame_split* split, uint32_t c, const rh_schema* s, uint64_t num_chunks, const rh_opts* opts,
                          struct ArrowArray* out_chunks, uint32_t* out_k, rh_stats* stats, char** err);
void rh_frame_split_free(rh_frame_split* split);
void rh_frame_last(float* classify_ms, float* scan_offsets_ms, float* gather_ms, uint64_t* n);

/* Framed messages, the write side (symbols added without a change of RH_ABI_VERSION: look them up by name).
 * rh_frame_join: the datums of `nsrc` sources -- each one chunk of a device-resident encode result -- become n messages, every
 * datum behind the header of `framing` that carries its source's wire id, produced in HBM.  Without indices the messages are the
 * sources' rows in the order given; with indices (host memory, one int64 per row of that chunk, on every source that has rows or
 * on none) row j of a source becomes message indices[j], and the indices together must be a permutation of 0 .. n-1.  n must be
 * the rows of all sources together; the sources live on one device.  The result is an rh_device_encoded of
 * rh_clamp_chunks(n, num_chunks) BinaryArrays, chunked as rh_encode chunks n rows: rh_device_encoded_export / _to_host /
 * _output_bytes / _free apply.  The sources are read, not consumed.  The source table lies in device memory: nsrc is not bounded by
 * kernel-argument space.
 * Failures (RH_ERR_DECODE, the message starts with "framed: "): the first index outside 0 .. n-1 (the lowest source row in the
 * order given) "schema id {id}: index {v} is outside 0 .. {n-1}"; else the lowest position that is not named exactly once,
 * "position {p} is named more than once" / "position {p} is never named"; a chunk whose messages pass 2^31-1 bytes names the
 * chunk.  rh_opts.devices and RH_ASYNC are refused with RH_ERR_ARGUMENT.
 * rh_frame_join_last: GPU time of the most recent join's lengths kernel, of its three prefix kernels, and of its gather. */
typedef struct rh_frame_source {
  const rh_device_encoded* enc;
  uint32_t chunk;
  uint32_t pad;
  uint64_t id;              /* the wire id, unsigned (a confluent id lies in 0 .. 2^32-1) */
  const int64_t* indices;   /* host, one per row of that chunk, or NULL */
} rh_frame_source;
int rh_frame_join(const rh_frame_source* src, uint32_t nsrc, uint32_t framing, uint64_t n, uint64_t num_chunks, const rh_opts* opts,
                  rh_device_encoded** out, char** err);
void rh_frame_join_last(float* lengths_ms, float* scan_ms, float* gather_ms, uint64_t* n);

/* Measurement hook, not part of the drop-in surface: the host-side gather of a `shards`-GPU rh_decode call (every shard's
 * record slices copied into its staging buffer by its own host thread + `threads_per_shard` helpers, all shards at once)
 * without the GPUs -- pageable destinations (pinned = 0, runs on a box with no device), pinned ones (1), or pageable ones placed
 * per NUMA node with the shard's threads bound there (2; rh_numa_nodes() = how many nodes the kernel shows).  *best_ms = best
 * wall time of `reps` rounds; returns the payload bytes per round, 0 on failure.  scripts/gather_scaling.py. */
uint64_t rh_bench_gather(const uint8_t* const* ptrs, const uint64_t* lens, uint64_t n, uint32_t shards,
                         uint32_t threads_per_shard, int pinned, uint32_t reps, double* best_ms);
uint32_t rh_numa_nodes(void);

/* Test hook, not part of the drop-in surface: exercises the host thread pool behind the gather of pipelined calls (its
 * lock-free phase hand-over); 0 = every task of every phase ran exactly once.  tests/test_host.py. */
uint32_t rh_selftest_pool(uint32_t workers, uint32_t phases, uint32_t max_tasks);

void rh_free_string(char* s);
int rh_abi_version(void);
/* CPUs the process may use: hardware threads cut down to its affinity mask and its cgroup CPU quota -- what the engine
 * sizes its host thread pools by, and what a binding should size its own by (the CPython boundary's extractor threads do). */
uint32_t rh_effective_cpus(void);
/* Number of visible HIP devices (0 when no GPU / driver); never throws. */
int rh_device_count(void);
/* The calling thread's current HIP device (what rh_opts.device = -1 resolves to on this thread), or -1 when there is
 * none.  The current device is per host thread: a binding that moves a call to a thread of its own resolves -1 with
 * this BEFORE it starts the thread (the CPython boundary does, pymodule.cpp).  Never throws. */
int rh_current_device(void);

#ifdef __cplusplus
}
#endif
#endif
