"""Framed writes, the part that needs no device: the entry points exist beside an unchanged ABI and unchanged kernel-cache keys,
``serialize_framed`` is one object under both module names, every refusal that is raised before any device work carries its exact
message, and the CPU check of csrc/frame_join_core.h builds and passes."""
import subprocess

import numpy as np
import pytest

import frame_cases as FR
from avrogen import synth
from avrogen.schemas import SCHEMAS
from oracle import c_walker
from test_projection import PARENT_KEYS

import pyruhvro
import pyruhvro_amd as P
from pyruhvro_amd import cabi

FULL = SCHEMAS["full"]
BATCH = c_walker.decode(synth.records("full", 4, seed=2), FULL)      # 4 rows, made by the oracle


def _raises(exc, message, f):
    with pytest.raises(exc) as e:
        f()
    if message is not None:
        assert str(e.value) == message, str(e.value)
    return str(e.value)


def test_symbols_exist_the_abi_is_still_7_and_the_kernel_keys_are_the_parents():
    L = cabi.lib()
    assert L.rh_abi_version() == 7
    assert set(cabi.FRAME_JOIN_SYMBOLS) == {"rh_encode_to_device", "rh_frame_join", "rh_frame_join_last"}
    for name in cabi.FRAME_JOIN_SYMBOLS:
        assert getattr(L, name, None) is not None, name
        assert cabi._frame_join_sym(name).argtypes is not None
    for name, key in PARENT_KEYS.items():
        assert cabi.kernel_key(SCHEMAS[name]) == key, name
        assert cabi.kernel_key(SCHEMAS[name], encode=True) == cabi.kernel_key(SCHEMAS[name], True)
    assert set(cabi.frame_join_last()) == {"lengths_ms", "scan_ms", "gather_ms", "n"}


def test_one_object_under_both_module_names():
    assert "serialize_framed" in P.__all__ and "serialize_framed" in pyruhvro.__all__
    assert pyruhvro.serialize_framed is P.serialize_framed
    from pyruhvro_amd import framing
    assert P.serialize_framed is framing.serialize_framed
    assert sorted(pyruhvro.__all__) == sorted(set(pyruhvro.__all__))
    for name in pyruhvro.__all__:
        assert getattr(pyruhvro, name) is getattr(P, name), name


# ---- refusals, all before any device work (this file runs without a device) ---------------------------------------------------------
def test_unknown_framing():
    _raises(ValueError, "framed: unknown framing 'kafka' (one of 'confluent', 'single_object')",
            lambda: P.serialize_framed([(1, FULL, BATCH)], 1, framing="kafka"))
    _raises(ValueError, "framed: unknown framing None (one of 'confluent', 'single_object')",
            lambda: P.serialize_framed([(1, FULL, BATCH)], 1, framing=None))


def test_zero_groups_or_more_than_32():
    _raises(ValueError, "framed: 1 to 32 groups per call", lambda: P.serialize_framed([], 1))
    _raises(ValueError, "framed: 1 to 32 groups per call", lambda: P.serialize_framed([(i, FULL, BATCH) for i in range(33)], 1))


@pytest.mark.parametrize("key", ["1", 1.0, True, None, (1,), b"\x01"], ids=["str", "float", "bool", "None", "tuple", "bytes"])
def test_an_id_that_is_not_an_int(key):
    for framing in FR.FRAMINGS:
        _raises(ValueError, f"framed: schema id {key!r} is not an int", lambda: P.serialize_framed([(key, FULL, BATCH)], 1, framing=framing))


@pytest.mark.parametrize("framing,key", [("confluent", -1), ("confluent", 1 << 32), ("confluent", 1 << 63), ("single_object", 1 << 64),
                                         ("single_object", -(1 << 63) - 1)])
def test_an_id_out_of_range_for_the_framing(framing, key):
    lo, bits = (0, 32) if framing == "confluent" else (-(1 << 63), 64)
    _raises(ValueError, f"framed: schema id {key} is out of range for the {framing} framing ({lo} .. 2**{bits}-1)",
            lambda: P.serialize_framed([(key, FULL, BATCH)], 1, framing=framing))


def test_two_groups_with_one_id_on_the_wire():
    _raises(ValueError, "framed: two keys of schemas are the same schema id on the wire",
            lambda: P.serialize_framed([(7, FULL, BATCH), (7, FULL, BATCH)], 1))
    _raises(ValueError, "framed: two keys of schemas are the same schema id on the wire",
            lambda: P.serialize_framed([(-1, FULL, BATCH), ((1 << 64) - 1, FULL, BATCH)], 1, framing="single_object"))


def test_a_schema_the_encoder_does_not_take():
    for bad in ("{nope", '{"type": "record", "name": "R", "fields": [{"name": "x", "type": "nope"}]}'):
        plain = _raises(ValueError, None, lambda: P.serialize_record_batch(BATCH, bad, 1))
        _raises(ValueError, f"framed: schema id 9: {plain}", lambda: P.serialize_framed([(3, FULL, BATCH), (9, bad, BATCH)], 1))
    # a negative single-object key is reported as the id the wire carries
    plain = _raises(ValueError, None, lambda: P.serialize_record_batch(BATCH, "{nope", 1))
    _raises(ValueError, f"framed: schema id {(1 << 64) - 2}: {plain}", lambda: P.serialize_framed([(-2, "{nope", BATCH)], 1, framing="single_object"))


def test_indices_on_some_groups_only():
    idx = np.arange(4, dtype=np.int64)
    message = "framed: indices are given for some groups and not for others"
    _raises(ValueError, message, lambda: P.serialize_framed([(1, FULL, BATCH, idx), (2, FULL, BATCH)], 1))
    _raises(ValueError, message, lambda: P.serialize_framed([(1, FULL, BATCH, None), (2, FULL, BATCH, idx + 4)], 1))
    _raises(ValueError, message, lambda: P.serialize_framed([P.FramedGroup(1, FULL, idx, [BATCH]), (2, FULL, [BATCH])], 1))


def test_the_wrong_number_of_indices():
    _raises(ValueError, "framed: schema id 2 has 8 rows and 4 indices",
            lambda: P.serialize_framed([(1, FULL, BATCH, [0, 1, 2, 3]), (2, FULL, [BATCH, BATCH], [4, 5, 6, 7])], 1))
    _raises(ValueError, "framed: schema id 1 has 0 rows and 1 indices", lambda: P.serialize_framed([(1, FULL, [], [0])], 1))
    _raises(ValueError, "framed: schema id 5 has 4 rows and 0 indices",
            lambda: P.serialize_framed([P.FramedGroup(5, FULL, np.zeros(0, dtype=np.int64), [BATCH])], 1))


def test_more_than_one_device_is_refused():
    old = P.set_devices([0, 0])
    try:
        msg = _raises(ValueError, None, lambda: P.serialize_framed([(1, FULL, BATCH)], 1))
        assert msg.startswith("framed: ") and "one device" in msg
    finally:
        P.set_devices(old)


def test_type_errors():
    for groups in (((1, FULL, BATCH),), {1: (FULL, BATCH)}, None, BATCH, iter([(1, FULL, BATCH)])):
        _raises(TypeError, "argument 'groups': expected a list of groups", lambda: P.serialize_framed(groups, 1))
    for group in ([1, FULL, BATCH], (1, FULL), (1, FULL, BATCH, None, None), 1, None, {"id": 1}):
        assert _raises(TypeError, None, lambda: P.serialize_framed([(2, FULL, BATCH), group], 1)).startswith("argument 'groups': group 1 ")
    for batches in (None, 5, "batch", [BATCH, None], BATCH.to_struct_array(), [BATCH.column(0)]):
        assert _raises(TypeError, None, lambda: P.serialize_framed([(1, FULL, batches)], 1)).startswith("argument 'groups': group 0")
    for indices in ([0.5, 1, 2, 3], "0123", [[0, 1], [2, 3]], np.zeros(4, dtype=np.float64)):
        assert _raises(TypeError, None, lambda: P.serialize_framed([(1, FULL, BATCH, indices)], 1)).startswith("argument 'groups': group 0")
    _raises(TypeError, None, lambda: P.serialize_framed([(1, 5, BATCH)], 1))
    _raises(TypeError, None, lambda: P.serialize_framed([(1, FULL, BATCH)], "2"))
    _raises(OverflowError, None, lambda: P.serialize_framed([(1, FULL, BATCH)], -1))


# ---- the CPU check -------------------------------------------------------------------------------------------------------------------------
def test_the_build_recipe_runs_frame_join_check():
    from pyruhvro_amd import _build
    exe = _build.build_frame_join_check()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("frame_join_check: ") and last.endswith(" 0 failures"), last
    assert "build_frame_join_check" in open(_build.ROOT + "/__graft_entry__.py").read()
    for name in ("frame_join.hip", "engine_frame_join.cpp"):
        assert name in _build.LIB_SOURCES and name in _build.LIB_DEPS
    for name in ("frame_join.h", "frame_join_core.h"):
        assert name in _build.LIB_DEPS
