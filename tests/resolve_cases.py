"""Test side of reader schemas: the Avro 1.11 "Schema Resolution" mapping on VALUES, reader-schema builders and the cases the
GPU tests of tests/test_resolution.py decode (scripts/known_schemas.py prebuilds their kernels).

``resolve_record(W, R, value)`` maps a value written under W to the value a reader of R sees; the expected batches are the
oracle's decode under R of ``to_datum(R, resolve_record(...))`` -- never the engine's own output."""
import json
import random

import numpy as np

from avrogen.encoder import Blocks, Branch, _fits, to_datum
from avrogen.schemas import SCHEMAS
from oracle.avro_schema import parse_schema

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
INT_TYPES = ("int", "long")
PROMOTIONS = {"int": ("long", "float", "double"), "long": ("float", "double"), "float": ("double",), "string": ("bytes",), "bytes": ("string",)}


def _leaf(w, r, v):
    if w.kind == r.kind:
        return v
    if w.kind in INT_TYPES and r.kind == "long":
        return v
    if w.kind in INT_TYPES and r.kind == "float":
        return float(np.array(v, np.int64).astype(np.float32))       # ONE rounding, to nearest even
    if w.kind in INT_TYPES and r.kind == "double":
        return float(np.array(v, np.int64).astype(np.float64))
    if w.kind == "float" and r.kind == "double":
        return float(np.float32(v).astype(np.float64)) if v == v else _nan64(v)
    if w.kind == "string" and r.kind == "bytes":
        return v if isinstance(v, bytes) else v.encode()
    if w.kind == "bytes" and r.kind == "string":
        return bytes(v)                                               # (the encoder writes a bytes "string" as it is)
    raise AssertionError((w.kind, r.kind))


def _nan64(v):
    import struct
    return float(np.frombuffer(struct.pack("<f", v), np.float32).astype(np.float64)[0])


def resolve(w, r, v):
    """The value `v` of writer type `w` as reader type `r` sees it (both oracle AvroSchema nodes, structurally matching)."""
    if w.kind == "union":
        if isinstance(v, Branch):
            i, inner = v.idx, v.value
        else:
            i = next(i for i, var in enumerate(w.variants) if _fits(var, v))
            inner = v
        return Branch(i, resolve(w.variants[i], r.variants[i], inner))
    if w.kind == "record":
        return {f.name: resolve(f.schema, g.schema, v[f.name]) for f, g in zip(w.fields, r.fields)}
    if w.kind in ("array", "map") and isinstance(v, Blocks):      # (an explicit block structure is kept: the columns do not depend on it)
        one = (lambda it: (it[0], resolve(w.items, r.items, it[1]))) if w.kind == "map" else (lambda it: resolve(w.items, r.items, it))
        return Blocks([([one(it) for it in items], with_size) for items, with_size in v.blocks])
    if w.kind == "array":
        return [resolve(w.items, r.items, x) for x in v]
    if w.kind == "map":
        items = list(v.items()) if isinstance(v, dict) else list(v)
        return [(k, resolve(w.items, r.items, x)) for k, x in items]
    return _leaf(w, r, v)


def _default_value(t, d):
    if t.kind == "union":
        return Branch(0, _default_value(t.variants[0], d))
    if t.kind == "bytes":
        return d.encode("latin-1")
    if t.kind in ("float", "double"):
        return float(d)
    return d


def resolve_record(wj: str, rj: str, value: dict) -> dict:
    w, r = parse_schema(wj), parse_schema(rj)
    wf = {f.name: f for f in w.fields}
    defaults = {f["name"]: f.get("default") for f in json.loads(rj)["fields"]}
    out = {}
    for f in r.fields:
        if f.name in wf:
            out[f.name] = resolve(wf[f.name].schema, f.schema, value[f.name])
        else:
            out[f.name] = _default_value(f.schema, defaults[f.name])
    return out


def writer_records(wj, values):
    w = parse_schema(wj)
    return [to_datum(w, v) for v in values]


def reader_records(wj, rj, values):
    r = parse_schema(rj)
    return [to_datum(r, resolve_record(wj, rj, v)) for v in values]


# ---- reader-schema builders ------------------------------------------------------------------------------------------------------
def promote_type(t, pick):
    """The type `t` (schema JSON) with every promotable leaf replaced by pick(kind) (None: keep), at any depth."""
    if isinstance(t, str):
        return (pick(t) or t) if t in PROMOTIONS else t
    if isinstance(t, list):
        return [promote_type(x, pick) for x in t]
    t = dict(t)
    if "logicalType" in t:
        return t
    if t["type"] == "record":
        t["fields"] = [dict(f, type=promote_type(f["type"], pick)) for f in t["fields"]]
    elif t["type"] == "array":
        t["items"] = promote_type(t["items"], pick)
    elif t["type"] == "map":
        t["values"] = promote_type(t["values"], pick)
    elif t["type"] in PROMOTIONS:
        t["type"] = pick(t["type"]) or t["type"]
    return t


def make_reader(wj, keep=None, promote=None, add=(), name=None):
    """Reader schema from writer schema `wj`: `keep` top-level fields in that order (None: all), leaves promoted by
    `promote` (kind -> kind or None), `add` = [(position, field dict with default)]."""
    j = json.loads(wj)
    by = {f["name"]: f for f in j["fields"]}
    fields = [dict(by[n]) for n in (keep if keep is not None else [f["name"] for f in j["fields"]])]
    if promote:
        fields = [dict(f, type=promote_type(f["type"], promote)) for f in fields]
    for pos, f in sorted(add, key=lambda x: x[0]):
        fields.insert(min(pos, len(fields)), f)
    j["fields"] = fields
    if name:
        j["name"] = name
    return json.dumps(j)


ADD_ALL = [
    {"name": "d_null", "type": ["null", "long"], "default": None},
    {"name": "d_bool", "type": "boolean", "default": True},
    {"name": "d_int", "type": "int", "default": -77},
    {"name": "d_long", "type": "long", "default": 1234567890123456789},
    {"name": "d_float", "type": "float", "default": 1.5},
    {"name": "d_double", "type": "double", "default": -2.25e100},
    {"name": "d_str", "type": "string", "default": "unknown"},
    {"name": "d_empty", "type": "string", "default": ""},
    {"name": "d_bytes", "type": "bytes", "default": "aÿb\u0080"},
    {"name": "d_enum", "type": {"type": "enum", "name": "Colour", "symbols": ["RED", "GREEN", "BLUE"]}, "default": "GREEN"},
    {"name": "d_optstr", "type": ["string", "null"], "default": "dflt"},
]

# ---- promotions ------------------------------------------------------------------------------------------------------------------
PROMO_W = json.dumps({"type": "record", "name": "Promo", "fields": [
    {"name": "i", "type": "int"}, {"name": "l", "type": "long"}, {"name": "f", "type": "float"},
    {"name": "ni", "type": ["null", "int"]}, {"name": "ln", "type": ["long", "null"]}, {"name": "nf", "type": ["null", "float"]},
    {"name": "rec", "type": {"type": "record", "name": "PromoIn", "fields": [
        {"name": "a", "type": "int"}, {"name": "b", "type": ["null", "long"]}, {"name": "c", "type": "float"}, {"name": "s", "type": "string"}]}},
    {"name": "ai", "type": {"type": "array", "items": "int"}}, {"name": "al", "type": {"type": "array", "items": "long"}},
    {"name": "af", "type": {"type": "array", "items": ["null", "float"]}},
    {"name": "mi", "type": {"type": "map", "values": "int"}}, {"name": "ml", "type": {"type": "map", "values": "long"}},
    {"name": "u", "type": ["string", "int", "boolean"]}, {"name": "u2", "type": ["boolean", "float", "null"]},
    {"name": "v", "type": ["boolean", "long", "null"]},
    {"name": "s", "type": "string"}, {"name": "by", "type": ["null", "bytes"]}]})
PROMO_PICKS = {
    "a": {"int": "long", "long": "float", "float": "double", "string": "bytes", "bytes": "string"},
    "b": {"int": "float", "long": "double"},
    "c": {"int": "double", "long": "float", "float": "double"},
}
INTS = [I32_MIN, I32_MAX, 0, -1, 1, (1 << 24) + 1, -((1 << 24) + 1), 63, 64, -65, 1 << 27, -(1 << 28) - 1, 123456789]      # 1..5 byte varints
LONGS = [I64_MIN, I64_MAX, (1 << 53) + 1, -((1 << 53) + 1), (1 << 60) + (1 << 36) + 1, -((1 << 60) + (1 << 36) + 1), 0, -1, 1 << 34,
         (1 << 24) + 1, 1 << 62, -(1 << 48) - 3, 5]                                                                       # up to 10 byte varints
FLOATS = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), 3.4028234663852886e38, -3.4028234663852886e38, 1.1754943508222875e-38,
          1e-45, -8.407790785948902e-45, 1.5, -2.75, 16777217.0]                                                            # (1e-45: a float32 subnormal)


def promo_values(n, seed=7):
    r = random.Random(seed)
    out = []
    for k in range(n):
        i, l, f = INTS[k % len(INTS)], LONGS[k % len(LONGS)], FLOATS[k % len(FLOATS)]
        ri = lambda: r.choice(INTS) if r.random() < 0.5 else r.randint(I32_MIN, I32_MAX)      # noqa: E731
        rl = lambda: r.choice(LONGS) if r.random() < 0.5 else r.randint(I64_MIN, I64_MAX)     # noqa: E731
        rf = lambda: r.choice(FLOATS)                                                         # noqa: E731
        out.append({
            "i": i, "l": l, "f": f,
            "ni": None if k % 3 == 0 else ri(), "ln": None if k % 4 == 1 else rl(), "nf": None if k % 5 == 2 else rf(),
            "rec": {"a": ri(), "b": None if k % 2 else rl(), "c": rf(), "s": "r%d" % k},
            "ai": [ri() for _ in range(k % 5)], "al": [rl() for _ in range((k * 7) % 4)],
            "af": [None if (k + j) % 3 == 0 else rf() for j in range(k % 4)],
            "mi": [("k%d" % j, ri()) for j in range(k % 3)], "ml": [("key%d" % j, rl()) for j in range((k + 1) % 3)],
            "u": [("s%d" % k), ri(), bool(k & 1)][k % 3], "u2": [bool(k & 1), rf(), None][(k + 1) % 3],
            "v": [True, rl(), None][k % 3],
            "s": "x" * (k % 11), "by": None if k % 2 else bytes([k % 128, 0xC3, 0xA9]),      # (valid UTF-8: one reader takes it as a string)
        })
    return out


def promo_reader(which):
    m = PROMO_PICKS[which]
    return make_reader(PROMO_W, promote=lambda k: m.get(k))


# ---- defaults ---------------------------------------------------------------------------------------------------------------------
DEF_W = json.dumps({"type": "record", "name": "Def", "fields": [
    {"name": "id", "type": "long"}, {"name": "name", "type": ["null", "string"]}, {"name": "n", "type": "int"}]})


def def_values(n):
    return [{"id": k * 1_000_003, "name": None if k % 3 == 0 else "n%d" % k, "n": k - 5} for k in range(n)]


def def_readers():
    front = make_reader(DEF_W, add=[(0, f) for f in ADD_ALL[:4]] + [(2 + 4, f) for f in ADD_ALL[4:8]] + [(99, f) for f in ADD_ALL[8:]])
    one_kept = make_reader(DEF_W, keep=["name"], add=[(0, f) for f in ADD_ALL[:5]] + [(99, f) for f in ADD_ALL[5:]])
    return {"spread": front, "one_kept": one_kept}


# ---- `full`: a dropped, reordered, added and promoted mix ---------------------------------------------------------------------------
FULL_MIXED = make_reader(SCHEMAS["full"], keep=["class", "created_at", "name", "status", "age", "emails"],
                         promote=lambda k: {"int": "long", "long": "double"}.get(k),
                         add=[(0, ADD_ALL[0]), (3, ADD_ALL[6]), (99, ADD_ALL[9])])
FULL_FIXED_ONLY = make_reader(SCHEMAS["full"], keep=["created_at", "age"], promote=lambda k: {"int": "long", "long": "double"}.get(k),
                              add=[(1, ADD_ALL[2])])      # K == 0 with a size pass (strings dropped)
FLAT_W = json.dumps({"type": "record", "name": "FlatL", "fields": [{"name": c, "type": "long"} for c in "abcd"]})
FLAT_R = make_reader(FLAT_W, promote=None, add=[(2, ADD_ALL[3])]).replace('{"name": "b", "type": "long"}', '{"name": "b", "type": "double"}')


def flat_values(n):
    return [{"a": k, "b": LONGS[k % len(LONGS)], "c": -k * (1 << 40), "d": I64_MAX - k} for k in range(n)]


def wide97_reader():
    j = json.loads(SCHEMAS["wide97"])
    names = [f["name"] for f in j["fields"]]
    r = random.Random(97)
    dropped = set(r.sample(names, 10))
    strs = [f["name"] for f in j["fields"] if f["name"] not in dropped and f["type"] in ("string", ["null", "string"])][:2]
    assert len(strs) == 2

    def pick_for(name):
        return (lambda k: "bytes" if k == "string" else None) if name in strs else None
    fields = [dict(f, type=promote_type(f["type"], pick_for(f["name"])) if pick_for(f["name"]) else f["type"]) for f in j["fields"] if f["name"] not in dropped]
    fields.insert(5, ADD_ALL[6])
    fields.append(ADD_ALL[0])
    j["fields"] = fields
    return json.dumps(j)


def mutate(schema_json, seed):
    """A seeded reader of a random schema: drop some top-level fields, shuffle, add two defaults, promote every promotable leaf
    with probability 1/2 (a union keeps its branches where a promotion would break the branch-for-branch rule)."""
    r = random.Random(5000 + seed)
    j = json.loads(schema_json)
    names = [f["name"] for f in j["fields"]]
    keep = [n for n in names if r.random() < 0.7] or names[:1]
    r.shuffle(keep)

    def pick(k):
        return r.choice(PROMOTIONS[k]) if r.random() < 0.5 else None

    def safe(t):
        p = promote_type(t, pick)
        try:
            _check_unions(t, p)
            return p
        except ValueError:
            return t
    by = {f["name"]: f for f in j["fields"]}
    fields = [dict(by[n], type=safe(by[n]["type"])) for n in keep]
    fields.insert(r.randint(0, len(fields)), ADD_ALL[r.randrange(0, 6)])
    fields.insert(r.randint(0, len(fields)), ADD_ALL[r.randrange(6, len(ADD_ALL))])
    j["fields"] = fields
    return json.dumps(j)


def _kind(t):
    return t if isinstance(t, str) else ("union" if isinstance(t, list) else (t.get("logicalType") or t["type"]))


def _matches(w, r):
    kw, kr = _kind(w), _kind(r)
    if kw == kr:
        try:
            _check_unions(w, r)
            return True
        except ValueError:
            return False
    return kr in PROMOTIONS.get(kw, ())


def _check_unions(w, r):
    """ValueError when some union of `r` does not resolve branch for branch against `w`."""
    if isinstance(w, list):
        prims = [x for x in r if isinstance(x, str)]
        if len(set(prims)) < len(prims):
            raise ValueError("duplicate branch")
        for i, b in enumerate(w):
            j = next((j for j, rb in enumerate(r) if _matches(b, rb)), None)
            if j != i:
                raise ValueError("union")
            _check_unions(b, r[i])
    elif isinstance(w, dict) and "logicalType" not in w:
        if w["type"] == "record":
            for f, g in zip(w["fields"], r["fields"]):
                _check_unions(f["type"], g["type"])
        elif w["type"] == "array":
            _check_unions(w["items"], r["items"])
        elif w["type"] == "map":
            _check_unions(w["values"], r["values"])


RANDOM_SEEDS = (1, 5, 9, 14, 22, 31)
ERROR_CASES = ("eob_mid_varint", "eob_f32", "bad_bool")
ERROR_READERS = ("drops_damaged", "promotes_damaged", "adds_default")


def error_cases():
    """Three of cases.error_cases() on the writer extended by a trailing long (test_projection.error_projection_cases)."""
    from test_projection import error_projection_cases
    picked = [c for c in error_projection_cases() if c[0] in ERROR_CASES]
    assert len(picked) == len(ERROR_CASES)
    return picked


def error_reader(wj, which):
    if which == "drops_damaged":
        return make_reader(wj, keep=["zz_tail"])
    if which == "promotes_damaged":
        return make_reader(wj, promote=lambda k: {"int": "long", "long": "double", "float": "double"}.get(k))
    return make_reader(wj, add=[(99, ADD_ALL[6])])


SLIDE_W = json.dumps({"type": "record", "name": "Slide", "fields": [
    {"name": "id", "type": "long"}, {"name": "pre", "type": ["null", "string"]}, {"name": "tags", "type": {"type": "array", "items": "string"}},
    {"name": "nums", "type": {"type": "array", "items": ["null", "int"]}}, {"name": "m", "type": {"type": "map", "values": "int"}},
    {"name": "post", "type": "string"}]})
SLIDE_R = make_reader(SLIDE_W, promote=lambda k: {"int": "long", "long": "double"}.get(k), add=[(1, ADD_ALL[6])])


def slide_values():
    """Records far larger than any LDS window (arrays of tens of thousands of items, the form of cases.giant_record_cases())
    between ordinary ones: a tile holds ranges that fit, ranges of one sliding record, and ordinary records again."""
    out = []
    for r in range(300):
        n = {3: 30_000, 64: 9_000, 65: 40_000, 299: 12_345}.get(r, [0, 1, 2, 5][r % 4])
        out.append({"id": r * 1_000_003 - 7, "pre": None if r % 3 == 0 else "P" * (r % 50),
                    "tags": ["tag-%d-%d" % (r, j) * (1 + j % 3) for j in range(n)],
                    "nums": [None if (r + j) % 5 == 0 else j * 7 - r for j in range(n // 2)],
                    "m": [("k%d" % j, I32_MAX - j) for j in range(min(n, 2000) // 4)], "post": "tail%d" % r})
    return out



def resolution_cases():
    """Every (writer, reader) pair the GPU tests decode with the specialised kernels."""
    import random_cases
    out = [(PROMO_W, promo_reader(w)) for w in sorted(PROMO_PICKS)]
    out += [(DEF_W, r) for r in def_readers().values()]
    out += [(SCHEMAS["full"], FULL_MIXED), (SCHEMAS["full"], FULL_FIXED_ONLY), (SCHEMAS["full_skewed"], FULL_MIXED), (FLAT_W, FLAT_R),
            (SCHEMAS["wide97"], wide97_reader())]
    out += [(random_cases.random_schema(s), mutate(random_cases.random_schema(s), s)) for s in RANDOM_SEEDS]
    out += [(c[1], error_reader(c[1], which)) for c in error_cases() for which in ERROR_READERS]
    out.append((SLIDE_W, SLIDE_R))
    return list(dict.fromkeys(out))
