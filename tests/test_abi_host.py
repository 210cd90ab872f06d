"""CPU: what rdst_amd/_lib.py derives from include/rdst_hip.h (argument types, struct layouts, constants) against
tests/golden/abi_signatures.json, which was recorded from the hand-written table the derivation replaced.  One wrong type is
silent on every import and shows only as a wrong result or a fault on the device, so the whole table is held, entry by entry.

    PYTHONPATH=<tree> python tests/test_abi_host.py --record   # rewrite the recording from the rdst_amd of <tree>

The recorder reads public names only (SIGNATURES, PackJob, LrSchedule, STEP_STATE_BYTES and the constants), so it runs against
the hand-written _lib.py as well as the derived one.
"""
import ctypes
import json
import os
import sys

import pytest

from rdst_amd import _lib, ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abi_signatures.json")
LIB_CONSTANTS = ("F32", "BF16", "F32X3", "EINVAL", "ENOTSUP", "ACT_NONE", "ACT_GELU", "ACT_LEAKY02", "ACT_LEAKY001",
                 "SKIP_LOSS", "SKIP_NONFINITE", "SKIP_PEER", "PREPACKED", "ABI_VERSION")
OPS_CONSTANTS = ("PACK_LINEAR", "PACK_CONV3_FWD", "PACK_LINEAR_SEC3", "PACK_LINEAR_X3", "PACK_CONV3_FWD_X3")


def type_name(ty):
    return "LrSchedule" if ty is _lib.LrSchedule else ty.__name__


def layout(struct):
    return {"size": ctypes.sizeof(struct),
            "fields": [[n, getattr(struct, n).offset, getattr(struct, n).size] for n, _ in struct._fields_]}


def snapshot():
    consts = {f"_lib.{k}": getattr(_lib, k) for k in LIB_CONSTANTS}
    consts.update({f"ops.{k}": getattr(ops, k) for k in OPS_CONSTANTS})
    consts["_lib.LrSchedule.MAX_MILESTONES"] = _lib.LrSchedule.MAX_MILESTONES
    return {"signatures": {n: [type_name(res), [type_name(a) for a in args]] for n, (res, args) in _lib.SIGNATURES.items()},
            "structs": {"PackJob": layout(_lib.PackJob), "LrSchedule": layout(_lib.LrSchedule)},
            "step_state_bytes": _lib.STEP_STATE_BYTES,
            "constants": consts}


@pytest.fixture(scope="module")
def recorded():
    return json.load(open(GOLDEN))


def test_signatures_equal_the_recording(recorded):
    got = snapshot()["signatures"]
    assert sorted(got) == sorted(recorded["signatures"])
    bad = {n: (recorded["signatures"][n], got[n]) for n in got if got[n] != recorded["signatures"][n]}
    assert not bad, bad
    # the classes themselves, not look-alikes: the call trace tests `ty is ctypes.c_void_p`
    by_name = {"c_int": ctypes.c_int, "c_long": ctypes.c_int64, "c_float": ctypes.c_float, "c_double": ctypes.c_double,
               "c_ulong": ctypes.c_size_t, "c_void_p": ctypes.c_void_p, "c_char_p": ctypes.c_char_p,
               "LP_c_int": ctypes.POINTER(ctypes.c_int), "LrSchedule": _lib.LrSchedule}
    for n, (res, args) in _lib.SIGNATURES.items():
        assert all(ty is by_name[type_name(ty)] for ty in (res, *args)), n


def test_every_parameter_has_a_name():
    assert set(_lib.PARAMS) == set(_lib.SIGNATURES)
    for n, (_, args) in _lib.SIGNATURES.items():
        assert len(_lib.PARAMS[n]) == len(args), n
        assert all(p.isidentifier() for p in _lib.PARAMS[n]), n
    assert _lib.PARAMS["rdst_wattn_fwd"] == ("qkv", "ld_qkv", "table", "mask", "mask_nw", "out", "ld_out", "B", "H", "W", "C",
                                             "heads", "ws", "shift", "scale", "dtype", "stream")
    assert _lib.PARAMS["rdst_abi_version"] == ()


def test_struct_layouts_equal_the_recording(recorded):
    got = snapshot()
    assert got["structs"] == recorded["structs"]
    assert [recorded["structs"][s]["size"] for s in ("PackJob", "LrSchedule")] == [64, 200]
    assert got["step_state_bytes"] == recorded["step_state_bytes"] == 48
    # rdst_step_state, field by field, as the header's comment lays it out
    assert [(n, getattr(_lib.StepState, n).offset) for n, _ in _lib.StepState._fields_] == [
        ("kept", 0), ("skipped", 8), ("last_keep", 16), ("last_reason", 20), ("last_clip", 24), ("last_lr", 28),
        ("last_sumsq", 32), ("reserved", 40)]


def test_constants_equal_the_recording(recorded):
    assert snapshot()["constants"] == recorded["constants"]


GOOD = """
/* a comment with a declaration inside: int rdst_ghost(int x); */
#ifndef T_H
#define T_H
#ifdef __cplusplus
extern "C" {
#endif
#define RDST_ONE 1   /* trailing
                        comment */
#define RDST_NEG (-7)
#define RDST_CAST ((size_t)-1)
typedef struct rdst_job { int kind; const float* W; int N, K; int64_t steps[3]; int32_t count; } rdst_job;
int rdst_version(void);
const char* rdst_text(void);
size_t rdst_bytes(int64_t n, double x);   // a line comment
int rdst_run(const rdst_job* jobs, rdst_job one, int* count, float s,
             const unsigned long long* seed, void* stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_reads_a_small_header():
    sig, params, structs, consts = _lib.parse_header(GOOD)
    job = structs["rdst_job"]
    assert consts == {"ONE": 1, "NEG": -7}
    assert [(n, getattr(job, n).offset, getattr(job, n).size) for n, _ in job._fields_] == [
        ("kind", 0, 4), ("W", 8, 8), ("N", 16, 4), ("K", 20, 4), ("steps", 24, 24), ("count", 48, 4)]
    assert sig == {"rdst_version": (ctypes.c_int, []), "rdst_text": (ctypes.c_char_p, []),
                   "rdst_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_double]),
                   "rdst_run": (ctypes.c_int, [ctypes.c_void_p, job, ctypes.POINTER(ctypes.c_int), ctypes.c_float,
                                               ctypes.c_void_p, ctypes.c_void_p])}
    assert params["rdst_run"] == ("jobs", "one", "count", "s", "seed", "stream")
    assert params["rdst_version"] == ()


@pytest.mark.parametrize("text, says", [
    ("int rdst_x(unsigned n, void* stream);", r"type 'unsigned' .* rdst_x"),                      # a type outside the map
    ("int rdst_x(const short* p);", r"type 'const short\*' .* rdst_x"),                           # ... behind a pointer
    ("float rdst_x(int n);", r"return type 'float' .* rdst_x"),
    ("int rdst_x(int n, float, void* stream);", r"without a name.* rdst_x"),                      # an unnamed parameter
    ("int rdst_x(const float*);", r"without a name.* rdst_x"),
    ("int rdst_x(int n); int rdst_count;", r"not a function declaration: int rdst_count"),        # no match
    ("int rdst_x(int n) { return n; }", r"not a function declaration"),
    ("typedef struct s { int a; short b; } s;", r"type 'short' .* struct s"),                     # a field outside the map
    ("typedef struct s { int a : 3; } s;", r"type 'int a :' .* struct s"),
    ("typedef struct s { float* a, b; } s;", r"cannot read the field"),
])
def test_parser_refuses_what_it_does_not_know(text, says):
    with pytest.raises(RuntimeError, match=says):
        _lib.parse_header(text)


def test_a_missing_header_is_named(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "HEADER_PATH", str(tmp_path / "include" / "rdst_hip.h"))
    with pytest.raises(RuntimeError, match=r"include/rdst_hip\.h is missing"):
        _lib._read_header()


if __name__ == "__main__" and "--record" in sys.argv:
    with open(GOLDEN, "w") as f:
        snap = snapshot()
        f.write('{"signatures": {\n' + ",\n".join(f"{json.dumps(n)}: {json.dumps(s)}" for n, s in snap["signatures"].items()))
        f.write('\n},\n"structs": ' + json.dumps(snap["structs"]) + ',\n"step_state_bytes": ' + str(snap["step_state_bytes"]))
        f.write(',\n"constants": ' + json.dumps(snap["constants"]) + "}\n")
    print("wrote", GOLDEN, "from", os.path.dirname(_lib.__file__))
