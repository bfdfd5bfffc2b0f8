"""Column projection: ``columns=[...]`` decodes only the requested top-level fields.

The contract: for any schema, record list, ``num_chunks`` and list ``cols`` of distinct top-level field names

    deserialize_array_threaded(recs, schema, k, columns=cols) == [b.select(cols) for b in <full decode>]

buffer for buffer, in the order asked for.  The expected value is always the ORACLE's full decode followed by
``RecordBatch.select`` -- never the engine's own full decode.  Errors are the full decode's, also when the damaged bytes belong
to a dropped field."""
import json
import os
import random
import re
import sys

import numpy as np
import pytest

import cases
import random_cases
from arrow_compare import assert_batches_identical
from avrogen import fastgen, synth
from avrogen.encoder import zigzag
from avrogen.schemas import SCHEMAS
from oracle import c_walker

import pyruhvro_amd as P
from pyruhvro_amd import cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"generic": cabi.KERNEL_GENERIC, "specialized": cabi.KERNEL_SPECIALIZED}

# kernel-cache keys of three un-projected schemas, taken on the commit before projection existed: the feature must not move them
# (the committed HBM-traffic stamp of profiles/hbm_traffic.json is the first one)
# (flat4 has no variable-length output, so no size pass: its generated source includes spec_flat.h since the emit kernels of such
#  schemas walk and count the tiles past the LDS window themselves -- its key moved once, 417c9ed0e24b0a1f before; the schemas
#  with counters, the benchmark's among them, keep theirs)
PARENT_KEYS = {"full": "d4e730578ea82b76", "cfg3": "082668f7bd568627", "flat4": "625c144b688e85ef"}

FULL_COLS = ["name", "age", "emails", "address", "phone_numbers", "preferences", "status", "created_at", "class"]
FULL_PROJECTIONS = [
    ["created_at"],                      # a single fixed column (K == 0)
    ["name"],                            # a single string; the first column only
    ["status"],                          # the union alone
    ["emails", "phone_numbers"],         # list + map only
    ["class"],                           # the last column only
    list(reversed(FULL_COLS)),           # everything, reversed
    ["created_at", "age"],               # K == 0
    ["name", "class"],
    ["name", "created_at", "class"],
]
ENTRY_COLS = ["created_at", "name", "emails"]       # the projection the other entry points are tried with


def _wide97_cols():
    names = [f["name"] for f in json.loads(SCHEMAS["wide97"])["fields"]]
    r = random.Random(97)
    return [names[i] for i in r.sample(range(len(names)), 12)]      # a dozen scattered columns, in no particular order


RANDOM_SEEDS = (1, 5, 9, 14, 22, 31)


def _random_projection(seed):
    schema = random_cases.random_schema(seed)
    names = [f["name"] for f in json.loads(schema)["fields"]]
    r = random.Random(1000 + seed)
    cols = r.sample(names, r.randint(1, len(names)))
    return schema, cols


def _with_tail(schema_json):
    """The schema with one more top-level field behind the others: a column that holds none of the bytes an error case damages."""
    s = json.loads(schema_json)
    s["fields"] = s["fields"] + [{"name": "zz_tail", "type": "long"}]
    return json.dumps(s)


def error_projection_cases():
    """cases.error_cases() on the schema extended by a trailing long: (name, schema, good records, bad record, message).  The good
    records carry the extra value; the bad record is the case's, unchanged (it fails inside the original fields)."""
    out = []
    for name, schema, goods, bad, msg in cases.error_cases():
        out.append((name, _with_tail(schema), [g + zigzag(7) for g in goods], bad, msg))
    return out


def projection_cases():
    """Every (schema, columns) the GPU tests below decode with the specialised kernels (scripts/known_schemas.py prebuilds them)."""
    out = [(SCHEMAS["full"], c) for c in FULL_PROJECTIONS + [ENTRY_COLS, ["class", "emails", "age"], ["emails"]]]
    out += [(SCHEMAS["array_and_map"], ["props"]), (SCHEMAS["array_and_map"], ["tags", "id"]), (SCHEMAS["t_union"], ["u"]),
            (SCHEMAS["t_nullable_nested"], ["inner"]), (SCHEMAS["wide97"], _wide97_cols()), (SCHEMAS["full_skewed"], ["created_at", "age"])]
    out += [_random_projection(seed) for seed in RANDOM_SEEDS]
    out += [(s, ["zz_tail"]) for s in dict.fromkeys(c[1] for c in error_projection_cases())]
    return out


@pytest.fixture(params=sorted(KERNELS))
def kernel(request):
    old = P.set_kernel_mode(request.param)
    yield KERNELS[request.param]
    P.set_kernel_mode(old)


def _expected(recs, schema, k, cols):
    return [b.select(cols) for b in c_walker.decode_threaded(recs, schema, k)]


def _same(got, exp):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        g.validate(full=True)
        assert g.schema.equals(e.schema, check_metadata=True)
        assert_batches_identical(g, e)


# ---- CPU: schema front-end, argument errors, program shape, kernel keys ----------------------------------------------------------
@pytest.mark.parametrize("name,cols", [("full", ["created_at", "age"]), ("full", list(reversed(FULL_COLS))), ("t_union", ["u"]),
                                       ("array_and_map", ["props", "id"]), ("wide97", None)])
def test_arrow_schema_of_a_projection_is_the_selected_full_schema(name, cols):
    import pyarrow as pa
    cols = cols or _wide97_cols()
    full = P.arrow_schema(SCHEMAS[name])
    exp = pa.schema([full.field(c) for c in cols], metadata=full.metadata)
    got = P.arrow_schema(SCHEMAS[name], columns=cols)
    assert got.names == cols
    assert got.equals(exp, check_metadata=True)
    for f, g in zip(exp, got):
        assert f.equals(g, check_metadata=True)
    assert P.arrow_schema(SCHEMAS[name], columns=None).equals(full, check_metadata=True)


@pytest.mark.parametrize("bad,word", [([], "empty"), (["nope"], "'nope'"), (["age", "age"], "'age'"), (["address.street"], "address.street"),
                                      (["age", 3], "3"), (["age", None], "None")])
def test_argument_errors_name_the_offender(bad, word):
    for f in (lambda: P.arrow_schema(SCHEMAS["full"], columns=bad),
              lambda: P.deserialize_array_threaded([b""], SCHEMAS["full"], 1, columns=bad),      # (raised before any GPU work)
              lambda: P.deserialize_array([b""], SCHEMAS["full"], columns=bad),
              lambda: cabi.kernel_key(SCHEMAS["full"], columns=bad)):
        with pytest.raises(ValueError) as e:
            f()
        assert word in str(e.value)
    if bad == ["address.street"]:
        with pytest.raises(ValueError, match="dotted path"):
            P.arrow_schema(SCHEMAS["full"], columns=bad)


def _spec_constants(src):
    m = re.search(r"static constexpr int K = (\d+), KL = (\d+), NDOM = (\d+), NBUF = (\d+), NNODES = (\d+), DEPTH = (\d+);", src)
    return dict(zip(("K", "KL", "NDOM", "NBUF", "NNODES", "DEPTH"), map(int, m.groups())))


def _op_literals(src):
    """The Ops of the generated walk: (code, flags, dom, a, b, c, buf0, buf1, buf2, node)."""
    out = []
    for m in re.finditer(r"Op op = \{(OP_\w+), ([^}]*)\}", src):
        out.append((m.group(1),) + tuple(int(x) for x in m.group(2).split(", ")))
    return out


def test_projected_program_shape():
    full = _spec_constants(cabi.kernel_source(SCHEMAS["full"]))
    # created_at: one non-null int64 buffer; age: validity + int32 values.  No counter, no child row domain.
    src = cabi.kernel_source(SCHEMAS["full"], columns=["created_at", "age"])
    k0 = _spec_constants(src)
    assert (k0["K"], k0["KL"], k0["NDOM"], k0["NBUF"], k0["NNODES"]) == (0, 0, 1, 3, 3)
    assert k0["DEPTH"] == full["DEPTH"]                       # the walk still nests as deep as the full schema's
    ops = _op_literals(src)
    # the same op sequence whatever is kept: every field is walked (compared with another projection that keeps no list --
    # the full schema's source repeats the bodies of its item-dense lists)
    assert [o[0] for o in ops] == [o[0] for o in _op_literals(cabi.kernel_source(SCHEMAS["full"], columns=["class", "name"]))]
    assert {o[0] for o in ops} >= {"OP_LIST_BEGIN", "OP_LIST_NEXT", "OP_LIST_TAIL", "OP_LIST_END", "OP_UNION_BEGIN", "OP_REC_BEGIN", "OP_ENUM"}
    kept = [o for o in ops if not (o[1] & 32)]
    assert [(o[0], o[6], o[7], o[9]) for o in kept] == [("OP_FIXED", 0, 1, 1), ("OP_FIXED", -1, 2, 2)]   # age (wire order), created_at
    for o in ops:
        if o[1] & 32:                                          # F_DROP: no buffer of a dropped column is named, no node
            assert o[6] == -1 and o[7] == -1 and o[9] == -1
            assert o[0] == "OP_LIST_NEXT" or o[8] == -1        # (LIST_NEXT keeps the min wire bytes per item in buf2)
    assert "walk_drop.h" in src and "DropCtx" in src
    assert "walk_drop.h" not in cabi.kernel_source(SCHEMAS["full"])
    # name (validity, offsets, data) + class (offsets, data): two byte counters, numbered densely
    src = cabi.kernel_source(SCHEMAS["full"], columns=["name", "class"])
    k2 = _spec_constants(src)
    assert (k2["K"], k2["KL"], k2["NDOM"], k2["NBUF"], k2["NNODES"]) == (2, 2, 1, 5, 3)
    kept = [o for o in _op_literals(src) if not (o[1] & 32)]
    assert sorted(b for o in kept for b in o[6:9] if b >= 0) == [0, 1, 2, 3, 4]
    assert sorted(o[3] for o in kept) == [0, 1]               # counter ids
    # the projected emit walk stops behind the last kept field where a size pass has checked the rest
    assert "if constexpr (EMIT) return;" in cabi.kernel_source(SCHEMAS["full"], columns=["name"])
    assert "if constexpr (EMIT) return;" not in cabi.kernel_source(SCHEMAS["full"], columns=["class"])


def test_kernel_keys_of_unprojected_schemas_do_not_move():
    assert cabi.lib().rh_abi_version() == 7
    assert hasattr(cabi.lib(), "rh_schema_project")
    for name, key in PARENT_KEYS.items():
        assert cabi.kernel_key(SCHEMAS[name]) == key
    assert cabi.kernel_key(SCHEMAS["full"], columns=["created_at", "age"]) != PARENT_KEYS["full"]
    assert cabi.kernel_key(SCHEMAS["full"], columns=FULL_COLS) != PARENT_KEYS["full"]
    assert cabi.kernel_key(SCHEMAS["full"], columns=["name"]) != cabi.kernel_key(SCHEMAS["full"], columns=["age"])
    assert json.load(open(os.path.join(ROOT, "profiles", "hbm_traffic.json")))["_kernel_key"] == PARENT_KEYS["full"]


def test_projection_is_decode_only():
    C = cabi.C
    L = cabi.lib()
    s = cabi.Schema.get(SCHEMAS["full"], ["age"])
    with pytest.raises(RuntimeError):
        cabi.kernel_key(SCHEMAS["full"], encode=True, columns=["age"])
    assert not L.rh_schema_encode_kernel_source(s.handle)
    # the C entry point refuses a projected schema with RH_ERR_ARGUMENT (4) before it looks at the batch or at a device
    arr, sch, out = cabi.ArrowArray(), cabi.ArrowSchema(), (cabi.ArrowArray * 1)()
    out_k, err = C.c_uint32(), C.c_char_p()
    L.rh_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p,
                            C.POINTER(C.c_char_p)]
    rc = L.rh_encode(s.handle, C.addressof(arr), C.addressof(sch), 1, None, out, C.byref(out_k), None, C.byref(err))
    assert rc == 4 and b"decode only" in err.value
    L.rh_free_string(C.cast(err, C.c_void_p))


def test_known_projections_lists_what_the_gpu_tests_decode():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import known_schemas
    known = {(s, tuple(c)) for s, c in known_schemas.known_projections()}
    assert {(s, tuple(c)) for s, c in projection_cases()} <= known
    for s, c in known:
        assert P.arrow_schema(s, columns=list(c)).names == list(c)


# ---- GPU: parity with the oracle's full decode + select -----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("cols", FULL_PROJECTIONS, ids=lambda c: "+".join(c) if len(c) < 4 else "reversed")
def test_full_projections(cols, k, kernel):
    recs = synth.records("full", 3001, seed=5)
    _same(P.deserialize_array_threaded(recs, SCHEMAS["full"], k, columns=cols), _expected(recs, SCHEMAS["full"], k, cols))
    if k == 1:
        g = P.deserialize_array(recs[:200], SCHEMAS["full"], columns=cols)
        _same([g], _expected(recs[:200], SCHEMAS["full"], 1, cols))


@pytest.mark.gpu
@pytest.mark.parametrize("name,cols", [("array_and_map", ["props"]), ("array_and_map", ["tags", "id"]), ("t_union", ["u"]),
                                       ("t_nullable_nested", ["inner"])])
def test_other_schemas(name, cols, kernel):
    if name in synth.GENERATORS:
        recs = synth.records(name, 2500, seed=3)
    else:
        recs = next(c[2] for c in cases.differential_cases() if c[1] == SCHEMAS[name]) * 150
    for k in (1, 3):
        _same(P.deserialize_array_threaded_spawn(recs, SCHEMAS[name], k, columns=cols), _expected(recs, SCHEMAS[name], k, cols))


@pytest.mark.gpu
def test_wide_schema_projection_switches_to_the_narrow_form(kernel):
    cols = _wide97_cols()
    assert "RH_WIDE_SCHEMA" in cabi.kernel_source(SCHEMAS["wide97"]) and "RH_WIDE_SCHEMA" not in cabi.kernel_source(SCHEMAS["wide97"], columns=cols)
    data, offsets = fastgen.generate("wide97", 1500)
    for k in (1, 4):
        got = cabi.decode_packed(data, offsets, SCHEMAS["wide97"], k, kernel=kernel, columns=cols)
        exp = c_walker.decode_packed(c_walker.CompiledSchema(SCHEMAS["wide97"]), data, offsets, k, threaded=True)
        _same(got, [b.select(cols) for b in exp])


@pytest.mark.gpu
@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_random_schemas_random_subsets(seed, kernel):
    schema, cols = _random_projection(seed)
    _, recs = random_cases.random_case(seed, 600)
    for k in (1, 5):
        _same(P.deserialize_array_threaded(recs, schema, k, columns=cols), _expected(recs, schema, k, cols))


@pytest.mark.gpu
def test_no_records_give_one_empty_batch_with_the_projected_schema(kernel):
    cols = ["class", "emails", "age"]
    got = P.deserialize_array_threaded([], SCHEMAS["full"], 4, columns=cols)
    assert len(got) == 1 and got[0].num_rows == 0 and got[0].schema.names == cols
    _same(got, _expected([], SCHEMAS["full"], 4, cols))


# ---- GPU: the other entry points ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_binary_array_and_device_entry_points(kernel):
    import pyarrow as pa
    import torch
    cols = ENTRY_COLS
    recs = synth.records("full", 4003, seed=8)
    exp = _expected(recs, SCHEMAS["full"], 3, cols)
    _same(P.deserialize_binary_array(pa.array(recs, type=pa.binary()), SCHEMAS["full"], 3, columns=cols), exp)
    dec = P.deserialize_to_device(recs, SCHEMAS["full"], 3, columns=cols)
    assert [b.schema.names for b in dec.batches] == [cols] * 3
    _same(dec.to_host(), exp)
    t = torch.from_dlpack(dec.batches[1].column("created_at").values)       # one kept column, consumed in place
    assert t.dtype == torch.int64 and t.cpu().numpy().tolist() == exp[1].column("created_at").to_pylist()
    dec.free()
    d, o = c_walker.pack(recs)
    _same(cabi.decode_packed(d, o, SCHEMAS["full"], 3, kernel=kernel, devices=[0, 0, 0], columns=cols), exp)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["async", "single_pass"])
def test_async_and_single_pass_forms(form, kernel):
    import torch
    cols = ["name", "created_at", "class"]
    n = 20_011
    recs = synth.records("full", n, seed=21)
    exp = _expected(recs, SCHEMAS["full"], 4, cols)
    d, o = c_walker.pack(recs)
    d_data = torch.zeros(len(d) + 64, dtype=torch.uint8, device="cuda:0")
    d_data[: len(d)].copy_(torch.from_numpy(d.copy()))
    d_off = torch.from_numpy(o.view(np.int64).copy()).to("cuda:0")
    kw = dict(device=0, stream=torch.cuda.current_stream().cuda_stream, kernel=kernel, columns=cols)
    cabi.decode_device(d_data.data_ptr(), d_off.data_ptr(), int(o[-1]), n, SCHEMAS["full"], 4, **kw).free()      # the size history
    rs = [cabi.decode_device(d_data.data_ptr(), d_off.data_ptr(), int(o[-1]), n, SCHEMAS["full"], 4, asynchronous=(form == "async"),
                             single_pass=(form == "single_pass"), **kw) for _ in range(3)]
    for r in rs:
        _same(r.to_host(), exp)
        r.free()


# ---- GPU: errors are the full decode's --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", error_projection_cases(), ids=lambda c: c[0])
def test_damage_in_a_dropped_field_raises_the_full_decodes_error(case, kernel):
    name, schema, goods, bad, msg = case
    recs = list(goods) + [bad] + list(goods)
    with pytest.raises(ValueError) as oracle_err:
        c_walker.decode_threaded(recs, schema, 2)
    assert msg in str(oracle_err.value)
    for k in (1, 2, len(recs)):
        with pytest.raises(ValueError) as e:
            P.deserialize_array_threaded(recs, schema, k, columns=["zz_tail"])       # a column that holds none of the damaged bytes
        assert str(e.value) == str(oracle_err.value)
    # ... and the undamaged records decode
    _same(P.deserialize_array_threaded(list(goods), schema, 2, columns=["zz_tail"]), _expected(list(goods), schema, 2, ["zz_tail"]))


@pytest.mark.gpu
def test_the_lowest_of_two_damaged_records_wins(kernel):
    recs = synth.records("full", 4000, seed=13)
    _same(P.deserialize_array_threaded(recs, SCHEMAS["full"], 4, columns=["created_at", "age"]),
          _expected(recs, SCHEMAS["full"], 4, ["created_at", "age"]))
    bad = list(recs)
    bad[1200] = b"\x02" + zigzag(-3)                  # chunk 1: name = string branch, negative length (a dropped field)
    bad[3500] = b"\x06"                               # chunk 3: an invalid branch byte for name
    with pytest.raises(ValueError) as oracle_err:
        c_walker.decode_threaded(bad, SCHEMAS["full"], 4)
    assert "negative string length" in str(oracle_err.value)
    for cols in (["created_at", "age"], ["class"], ["emails"]):
        with pytest.raises(ValueError) as e:
            P.deserialize_array_threaded(bad, SCHEMAS["full"], 4, columns=cols)
        assert str(e.value) == str(oracle_err.value)


# ---- GPU: K == 0 past the LDS window ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [cabi.KERNEL_AUTO, cabi.KERNEL_SPECIALIZED], ids=["auto", "specialized"])
def test_fixed_columns_of_records_past_the_window(mode, monkeypatch):
    """Only fixed-width columns of a schema with strings: no counter (K == 0), and 256 records of dropped strings do not fit an
    8 KiB window.  Such a projection keeps its size pass, which hands the tiles past the window to the ranged kernels."""
    import torch
    monkeypatch.setenv("RUHVRO_HIP_WIN_BYTES", "8192")
    cols = ["created_at", "age"]
    data, offsets = fastgen.generate("full_skewed", 30_011)
    n = len(offsets) - 1
    full = c_walker.decode_packed(c_walker.CompiledSchema(SCHEMAS["full_skewed"]), data, offsets, 5, threaded=True)
    exp = [b.select(cols) for b in full]
    _same(cabi.decode_packed(data, offsets, SCHEMAS["full_skewed"], 5, kernel=mode, columns=cols), exp)
    d_data = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda:0")
    d_data[: len(data)].copy_(torch.from_numpy(data.copy()))
    d_off = torch.from_numpy(offsets.view(np.int64).copy()).to("cuda:0")
    for _ in range(3):      # (from the second call on: a single-submission call, the one whose tile statistics are counted)
        c0 = cabi.engine_counters()
        r = cabi.decode_device(d_data.data_ptr(), d_off.data_ptr(), int(offsets[-1]), n, SCHEMAS["full_skewed"], 5, device=0,
                               stream=torch.cuda.current_stream().cuda_stream, kernel=mode, columns=cols)
        got = r.to_host()
        r.free()
        c1 = cabi.engine_counters()
        _same(got, exp)
    assert c1["over_window_tiles"] > c0["over_window_tiles"]
    if mode == cabi.KERNEL_SPECIALIZED:
        assert c1["subtiled_tiles"] - c0["subtiled_tiles"] == c1["over_window_tiles"] - c0["over_window_tiles"]


# ---- GPU: only the selected columns are produced ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_output_bytes(kernel):
    n = 10_000
    recs = synth.records("full", n, seed=2)
    _, full = P.deserialize_array_threaded_with_stats(recs, SCHEMAS["full"], 4)
    _, one = P.deserialize_array_threaded_with_stats(recs, SCHEMAS["full"], 4, columns=["created_at"])
    assert one["output_bytes"] == 8 * n                 # one non-null int64 column, no validity
    for cols in FULL_PROJECTIONS:
        if set(cols) == set(FULL_COLS):
            continue
        _, st = P.deserialize_array_threaded_with_stats(recs, SCHEMAS["full"], 4, columns=cols)
        assert 0 < st["output_bytes"] < full["output_bytes"], cols
