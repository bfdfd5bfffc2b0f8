"""Every schema whose specialised kernels should be in the kernel cache before a GPU run: the benchmark schemas plus
every schema the parity tests decode.  Lives outside the product package because it imports the test suite's case
tables (which use the oracle's schema model): build() and tests/conftest.py call it, pyruhvro_amd never does.

    python scripts/known_schemas.py        # prebuild all of them (hiprtc, gfx950; needs no GPU)
"""
import os
import sys
from typing import List

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def WIDE_SCHEMAS() -> List[str]:
    """The wide schemas (more than 64 scanned counters) once the engine takes them (round 6); [] while it refuses them."""
    from avrogen.schemas import SCHEMAS
    from pyruhvro_amd import cabi
    out = []
    for k, v in SCHEMAS.items():
        if k.startswith("wide"):
            try:
                cabi.Schema.get(v)
                out.append(v)
            except ValueError:
                pass
    return out


def known_schemas() -> List[str]:
    """Benchmark schemas + every schema the parity tests decode."""
    root = ROOT
    from avrogen.schemas import SCHEMAS
    out = [v for k, v in SCHEMAS.items() if not k.startswith("wide")] + WIDE_SCHEMAS()
    try:
        import json
        import cases
        for c in cases.wire_cases() + cases.nesting_cases() + cases.dense_list_cases() + cases.enum_form_cases() + cases.wide_counter_cases():
            out.append(c[1])
        for c in cases.wide_form_cases() + cases.giant_record_cases() + cases.deep_nesting_cases():
            out.append(c[1])
        for c in cases.error_cases():
            out.append(c[1])
        # tiles past the smallest LDS window (tests/test_form_switch.py; a case table without them has nothing to add)
        out += cases.form_switch_schemas() if hasattr(cases, "form_switch_schemas") else []
        for c in cases.differential_cases():
            out.append(c[1])
        out.append(cases.logical_case()[0])
        out += cases.encode_extra_schemas()
        out.append(cases.long_string_case(1)[0])
        import random_cases
        out += [random_cases.random_schema(seed) for seed in range(random_cases.PREBUILT_SEEDS)]
        import test_n4_types                      # SURVEY 8f N4 schemas
        out.append(test_n4_types.SCHEMA)
        out.append(test_n4_types.DUR_SCHEMA)
        import test_named_refs                    # named-type references (resolved by the front-end)
        out.append(test_named_refs.WITH_REFS)
        import damage                             # tolerant-decode fuzz (its other schemas are listed above)
        out.append(damage.LONG_PLACEHOLDER_SCHEMA)
        out.append(damage.UNION_NO_NULL_SCHEMA)
        g = json.load(open(os.path.join(root, "tests", "golden", "reference_vectors.json")))
        out += [json.dumps(s) for s in g["schemas"].values()]
    except ImportError:
        raise
    return out




def known_projections() -> list:
    """(schema, columns) pairs whose projected kernels (`columns=`: rh_schema_project) the GPU tests and
    scripts/projection_bench.py decode with: prebuilt by this script next to the schemas above."""
    from avrogen.schemas import SCHEMAS
    import test_projection
    out = [(s, tuple(c)) for s, c in test_projection.projection_cases()]
    out += [(SCHEMAS["full"], c) for c in (("created_at", "age"), ("name", "created_at", "class"), ("emails", "phone_numbers"))]
    out.append((SCHEMAS["full"], ("created_at", "name")))      # the tolerant tests' projection
    return list(dict.fromkeys(out))


def known_resolutions() -> list:
    """(writer, reader) pairs whose resolved kernels (`reader_schema=`: rh_schema_resolve) the GPU tests and
    scripts/resolution_bench.py decode with: prebuilt by this script next to the projections."""
    import resolve_cases
    import resolution_bench
    return list(dict.fromkeys(resolve_cases.resolution_cases() + [(resolution_bench.WRITER, r) for r in resolution_bench.readers().values()]))


def single_pass_schemas() -> List[str]:
    """The schemas whose single-pass kernel (rh_spec_fused) a bench line or a test runs: the only ones build() compiles it for --
    it is the most expensive of a schema's five kernels and opt-in; every other schema gets it on first request."""
    from avrogen.schemas import SCHEMAS
    import cases
    out = [SCHEMAS[k] for k in ("full", "cfg3", "flat4", "array_and_map", "nullable_primitives", "t_enum", "t_union")]
    if hasattr(cases, "form_switch_schemas"):      # (tests/test_form_switch.py: single pass -> two pass -> generic)
        out += [cases.form_switch_schema("id_str", "_single"), cases.form_switch_full_skewed_schema()]
    if hasattr(cases, "form_switch_full_wide_index_schema"):      # (single pass -> two pass -> wide indexing)
        out += [cases.form_switch_full_wide_index_schema(), cases.form_switch_full_wide_index_schema("_async")]
    return out


if __name__ == "__main__":
    from pyruhvro_amd.prebuild import prebuild_many
    with_fused = list(dict.fromkeys(single_pass_schemas()))
    rest = [s for s in dict.fromkeys(known_schemas()) if s not in set(with_fused)]
    rest.sort(key=len, reverse=True)            # (the widest schemas first: one of their kernels alone takes hiprtc minutes)
    os.environ["RUHVRO_HIP_PREBUILD_LEAN"] = "1"      # (the lean pair: for these schemas only -- the benchmark's and the lean tests')
    errs = prebuild_many(with_fused, verbose=True)
    os.environ["RUHVRO_HIP_PREBUILD_FUSED"] = "0"
    os.environ["RUHVRO_HIP_PREBUILD_LEAN"] = "0"
    errs += prebuild_many(rest, verbose=True)
    errs += prebuild_many(known_projections(), verbose=True)      # (without their single-pass kernel: compiled on first request)
    errs += prebuild_many([("resolve", w, r) for w, r in known_resolutions()], verbose=True)
    if not errs:
        from pyruhvro_amd.prebuild import mark_warm
        mark_warm(known_schemas())
    for e in errs:
        print(e[:2000])
    sys.exit(1 if errs else 0)
