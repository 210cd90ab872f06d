"""ctypes binding of librdst_hip.so (the C ABI of include/rdst_hip.h).  Fails loudly: there is no
fallback when the library is missing.

The header is the table: its declarations, structs and integer ``#define``s are parsed once at import, so the binding of
a new entry point is its declaration in include/rdst_hip.h and nothing else.  tests/test_abi_host.py pins what the parse
yields against a recording of the hand-written table it replaced."""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# RDST_HIP_LIB: load another build of the same C ABI (tools/ use it for the -DRDST_DEBUG library); the default
# is the in-tree release library, and a missing file raises either way
LIB_PATH = os.environ.get("RDST_HIP_LIB") or os.path.join(_HERE, "librdst_hip.so")
_INCLUDE = os.path.join(os.path.dirname(_HERE), "include")
HEADER_PATH = os.path.join(_INCLUDE, "rdst_hip.h")
# the side headers, prefix -> path: each gives the module <prefix>_HEADER_PATH, <prefix>_SIGNATURES and <prefix>_PARAMS
_SIDE_HEADERS = {"DATA": os.path.join(_INCLUDE, "rdst_hip_data.h"),             # the K-tap degradations (data.py)
                 "LRC": os.path.join(_INCLUDE, "rdst_hip_consistency.h"),       # LR consistency (loss/consistency.py)
                 "MSSSIM": os.path.join(_INCLUDE, "rdst_hip_msssim.h"),         # MS-SSIM (loss/msssim.py, metrics.py)
                 "NOISE": os.path.join(_INCLUDE, "rdst_hip_noise.h")}           # the noise term (data.py)

_SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
_FIELD_SCALARS = {**_SCALARS, "int32_t": C.c_int32}
_RETURNS = {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}
_POINTEES = {*_FIELD_SCALARS, "void", "char", "uint8_t", "unsigned long long"}   # what a pointer may point to, besides the structs


def _ctype(text, scalars, structs, where):
    """The ctypes class of one C type of the header; `structs` (by value, or pointed to) are the ones parsed so far."""
    ty = re.sub(r"\s*\*", "*", " ".join(text.split()))
    if ty == "int*":
        return C.POINTER(C.c_int)    # the one typed pointer: rdst_u_conv's host-side block count
    if ty.endswith("*") and ty[:-1].removeprefix("const ") in _POINTEES | set(structs):
        return C.c_void_p
    if ty in scalars or ty in structs:
        return scalars.get(ty) or structs[ty]
    raise RuntimeError(f"rdst_amd: include/rdst_hip.h: type '{ty}' is not in the binding's type map, in: {where}")


def _struct(name, body, structs):
    fields = []
    for stmt in filter(None, (" ".join(s.split()) for s in body.split(";"))):
        first, *more = (d.strip() for d in stmt.split(","))    # `int N, K`: the type stands before the first declarator
        m = re.fullmatch(r"(.+?)\s*\b(\w+)\s*(?:\[\s*(\d+)\s*\])?", first)
        rest = [re.fullmatch(r"()(\w+)\s*(?:\[\s*(\d+)\s*\])?", d) for d in more]
        if m is None or None in rest or (more and "*" in m[1]):
            raise RuntimeError(f"rdst_amd: include/rdst_hip.h: cannot read the field '{stmt}' of struct {name}")
        base = _ctype(m[1], _FIELD_SCALARS, structs, f"struct {name} {{ {stmt}; }}")
        fields += [(d[2], base * int(d[3]) if d[3] else base) for d in (m, *rest)]
    return type(name, (C.Structure,), {"_fields_": fields})


def parse_header(text):
    """(signatures, params, structs, constants) of a header text in the style of include/rdst_hip.h:
    name -> (restype, [argtypes]), name -> parameter names, typedef name -> ctypes.Structure, and the RDST_* ``#define``s
    whose value is an integer literal or a parenthesised negative one (without the prefix).  Strict: a declaration that
    does not match, a type outside the map or a parameter without a name raises and names the declaration."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants, lines = {}, []
    for line in text.splitlines():
        if not line.lstrip().startswith("#"):
            lines.append(line)
        elif m := re.fullmatch(r"\s*#\s*define\s+RDST_(\w+)\s+(\d+|\(\s*-\s*\d+\s*\))\s*", line):
            constants[m[1]] = int(re.sub(r"[()\s]", "", m[2]))
    body = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", "\n".join(lines), flags=re.S)
    structs = {}

    def cut(m):
        structs[m[2]] = _struct(m[2], m[1], structs)
        return ""
    body = re.sub(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;", cut, body, flags=re.S)
    signatures, params = {}, {}
    for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
        m = re.fullmatch(r"(.+?)\s*\b(\w+)\s*\((.*)\)", decl)
        if m is None:
            raise RuntimeError(f"rdst_amd: include/rdst_hip.h: not a function declaration: {decl}")
        ret = re.sub(r"\s*\*", "*", m[1])
        if ret not in _RETURNS:
            raise RuntimeError(f"rdst_amd: include/rdst_hip.h: return type '{ret}' is not in the binding's type map, in: {decl}")
        args = [] if m[3].strip() in ("", "void") else [re.fullmatch(r"(.+?)\s*\b(\w+)", a.strip()) for a in m[3].split(",")]
        if None in args:
            raise RuntimeError(f"rdst_amd: include/rdst_hip.h: a parameter without a name, in: {decl}")
        signatures[m[2]] = (_RETURNS[ret], [_ctype(a[1], _SCALARS, structs, decl) for a in args])
        params[m[2]] = tuple(a[2] for a in args)
    return signatures, params, structs, constants


def _read_header(path=None):
    path = path or HEADER_PATH
    if not os.path.exists(path):
        raise RuntimeError(f"rdst_amd: {path} is missing. The ctypes binding is derived from it "
                           "(it ships beside the package, as in the repository); there is no second copy.")
    with open(path) as f:
        return f.read()


# name -> (restype, argtypes) and name -> parameter names of every symbol include/rdst_hip.h declares (PARAMS is for tests
# and tools that pick arguments out of a call; the product path passes them by position)
SIGNATURES, PARAMS, _structs, CONSTANTS = parse_header(_read_header())

# the same of every side header: entry points outside ABI_VERSION's count (a library without them gets raisers)
_BOUND, _side_constants = dict(SIGNATURES), {}      # every symbol load() binds; the side headers' own constants
for _prefix, _path in _SIDE_HEADERS.items():
    _sigs, _params, _, _consts = parse_header(_read_header(_path))
    globals().update({_prefix + "_HEADER_PATH": _path, _prefix + "_SIGNATURES": _sigs, _prefix + "_PARAMS": _params})
    _BOUND.update(_sigs)
    _side_constants.update(_consts)
NOISE_HETERO, NOISE_RICIAN = _side_constants["NOISE_HETERO"], _side_constants["NOISE_RICIAN"]   # rdst_hip_noise.h's model numbers

PackJob = _structs["rdst_pack_job"]
LrSchedule = _structs["rdst_lr_schedule"]   # passed by value to rdst_adam_step_dev
LrSchedule.MAX_MILESTONES = dict(LrSchedule._fields_)["milestones"]._length_
StepState = _structs["rdst_step_state"]
STEP_STATE_BYTES = C.sizeof(StepState)

F32, BF16, F32X3 = (CONSTANTS[k] for k in ("F32", "BF16", "F32X3"))
EINVAL, ENOTSUP = CONSTANTS["EINVAL"], CONSTANTS["ENOTSUP"]
ACT_NONE, ACT_GELU, ACT_LEAKY02, ACT_LEAKY001 = (CONSTANTS[k] for k in ("ACT_NONE", "ACT_GELU", "ACT_LEAKY02", "ACT_LEAKY001"))
SKIP_LOSS, SKIP_NONFINITE, SKIP_PEER = (CONSTANTS[k] for k in ("SKIP_LOSS", "SKIP_NONFINITE", "SKIP_PEER"))

ABI_VERSION = 11             # must equal rdst_abi_version() of the loaded library (argument lists change between versions)
PREPACKED = (1 << 64) - 1   # RDST_PREPACKED ((size_t)-1): not an integer literal, so stated here

_lib = None


def load() -> C.CDLL:
    """Load the HIP library or raise: the product path never runs without it."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"rdst_amd: {LIB_PATH} is missing. Build it with `python -m rdst_amd.build` "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _BOUND.items():
        fn = getattr(lib, name, None)
        if fn is None:  # a declared symbol the .so does not export: calling it raises
            setattr(lib, name, _missing(name))
            continue
        fn.restype = res
        fn.argtypes = args
    got = lib.rdst_abi_version()
    if got != ABI_VERSION:   # a stale library would be called with shifted arguments (sizes read as pointers)
        raise RuntimeError(f"rdst_amd: {LIB_PATH} has ABI version {got}, this package binds version {ABI_VERSION}: "
                           "rebuild it with `python -m rdst_amd.build --force` (and `--debug` for the _dbg library)")
    _lib = lib
    return lib


def loaded() -> bool:
    return _lib is not None


def _missing(name):
    def raiser(*_a, **_k):
        raise RuntimeError(f"rdst_amd: {LIB_PATH} does not export {name}; rebuild with `python -m rdst_amd.build --force`")
    return raiser


class HipError(RuntimeError):
    pass


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().rdst_last_error().decode(errors="replace")
        raise HipError(f"{what} failed (rc={rc}): {msg}")
