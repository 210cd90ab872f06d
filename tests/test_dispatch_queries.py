"""The pure host queries of the C ABI (which fast path a shape takes, how much workspace its weight image needs) over a grid of
widths in every compute mode, against answers recorded from the library (tests/golden/dispatch_queries.json), and the refusal
of an unknown dtype by the entry points before they touch the device.  No GPU: the library loads without one.

    RDST_HIP_LIB=<lib> python tests/test_dispatch_queries.py --record   # rewrite the table from <lib>
"""
import ctypes
import itertools
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from rdst_amd import _lib  # noqa: E402

TABLE = os.path.join(HERE, "golden", "dispatch_queries.json")

DTYPES = (_lib.F32, _lib.BF16, _lib.F32X3, -1, 3)   # the three modes and two unknown values
# the E1 widths (60 / 90 / 120 and their qkv / fc1 / fusion / upsampler widths), ws16 (60), the SwinIR fixtures (48), the
# one-channel head / tail, and near misses
WIDTHS = (0, 1, 8, 30, 48, 59, 60, 61, 64, 90, 96, 120, 150, 180, 240, 270, 360)
HEADS = (1, 3, 6, 8)
WINDOWS = (4, 8, 16)
ACTS = (_lib.ACT_NONE, _lib.ACT_GELU, _lib.ACT_LEAKY02)
# the backward workspaces: token counts around the 32-row tile and at step size, pixel grids of one and of several tiles
TOKENS = (1, 31, 32, 33, 4096, 65536)
IMAGES = ((1, 8, 8), (1, 40, 32), (2, 64, 64))


def grids():
    """query name -> the argument tuples it is asked"""
    w2 = list(itertools.product(WIDTHS, WIDTHS))
    return {
        "rdst_conv_fwd_packable": [(ci, co, ks, r, res, act, dt) for ci, co in w2 for ks in (1, 3) for r in (1, 2, 3)
                                   for res in (0, 1) for act in ACTS for dt in DTYPES],
        "rdst_ln_linear_fwd_packable": [(k, n, ln, res, act, dt) for k, n in w2 for ln in (0, 1) for res in (0, 1) for act in ACTS
                                        for dt in DTYPES],
        "rdst_mlp_fwd_packable": [(c, h, dt) for c, h in w2 for dt in DTYPES],
        "rdst_mlp_fused_supported": [(c, h, dt) for c, h in w2 for dt in DTYPES],
        "rdst_swin_attn_fwd_supported": [(c, h, ws, dt) for c in WIDTHS for h in HEADS for ws in WINDOWS for dt in DTYPES],
        "rdst_conv_fwd_workspace2": [(ci, co, ks, dt) for ci, co in w2 for ks in (1, 3) for dt in DTYPES],
        "rdst_ln_linear_fwd_workspace2": [(k, n, dt) for k, n in w2 for dt in DTYPES],
        "rdst_ln_linear_bwd_workspace": [(m, k, n) for m in TOKENS for k, n in w2],
        "rdst_mlp_bwd_workspace": [(m, c, h) for m in TOKENS for c, h in w2],
        "rdst_conv_bwd_workspace": [(b, h, w, ci, co, ks) for b, h, w in IMAGES for ci, co in w2 for ks in (1, 3)],
        "rdst_wattn_bwd_workspace": [(b, h, w, c, hd, ws) for b, h, w in IMAGES for c in WIDTHS for hd in HEADS for ws in WINDOWS],
    }


def answers(lib, name):
    """the yes / no queries as a string of digits, the workspace sizes as a list"""
    got = [int(getattr(lib, name)(*args)) for args in grids()[name]]
    return "".join(map(str, got)) if name.endswith(("_packable", "_supported")) else got


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("name", sorted(grids()))
def test_query_answers_match_the_recorded_table(lib, name):
    want = json.load(open(TABLE))[name]
    got = answers(lib, name)
    assert len(want) == len(got)
    bad = [(args, w, g) for args, w, g in zip(grids()[name], want, got) if w != g]
    assert not bad, f"{len(bad)} answers moved, first: {bad[:5]}"


def test_fast_paths_are_reported_where_expected(lib):
    # spot checks of the table itself: the E1 shapes take the packed paths in bf16 and fp32x3, never in exact fp32
    for dt, want in ((_lib.BF16, 1), (_lib.F32X3, 1), (_lib.F32, 0)):
        assert lib.rdst_conv_fwd_packable(60, 60, 3, 1, 1, 0, dt) == want
        assert lib.rdst_conv_fwd_packable(60, 240, 3, 2, 0, 0, dt) == want
        assert lib.rdst_ln_linear_fwd_packable(60, 180, 1, 0, 0, dt) == want
    assert lib.rdst_ln_linear_fwd_packable(120, 60, 0, 1, _lib.ACT_GELU, _lib.F32X3) == 1   # fc2: fp32x3 only
    assert lib.rdst_ln_linear_fwd_packable(120, 60, 0, 1, _lib.ACT_GELU, _lib.BF16) == 0
    assert lib.rdst_mlp_fwd_packable(90, 180, _lib.BF16) == 1 and lib.rdst_mlp_fwd_packable(90, 180, _lib.F32X3) == 0
    assert lib.rdst_conv_fwd_workspace2(60, 60, 3, _lib.F32X3) > lib.rdst_conv_fwd_workspace2(60, 60, 3, _lib.BF16)


def _refusals(p):
    """(entry point, call with dtype d) on valid shapes and non-null pointers (a host buffer: nothing may be launched)"""
    z = 1 << 24
    return {
        "rdst_conv_fwd": lambda d: (p, 60, 0, p, p, None, 0, p, 60, p, z, 1, 32, 32, 60, 60, 3, 1.0, 1, d, None),
        "rdst_conv_bwd": lambda d: (p, 60, 0, p, p, 60, p, 60, None, 0, p, p, p, 1 << 40, 1, 32, 32, 60, 60, 3, 1.0, 1, d, None),
        "rdst_ln_linear_fwd": lambda d: (p, 60, p, p, 0, p, p, None, 0, p, 180, p, p, z, 64, 60, 180, 1.0, d, None),
        "rdst_ln_linear_bwd": lambda d: (p, 60, p, p, p, 0, p, p, 180, p, 60, None, 0, p, p, p, p, p, 1 << 40, 64, 60, 180, 1.0,
                                         d, None),
        "rdst_ln_linear_bwd2": lambda d: (p, 60, p, p, p, 0, p, p, 180, p, 60, None, 0, p, p, p, p, p, 1 << 40, 64, 60, 180, 1.0,
                                          d, None, None, 0),
        "rdst_wattn_fwd": lambda d: (p, 180, p, None, 0, p, 60, 1, 16, 16, 60, 6, 8, 0, 0.3, d, None),
        "rdst_wattn_bwd": lambda d: (p, 180, p, None, 0, p, 60, p, 180, p, p, 1 << 40, 1, 16, 16, 60, 6, 8, 0, 0.3, d, None),
        "rdst_wattn_fwd_drop": lambda d: (p, 180, p, None, 0, p, 60, 1, 16, 16, 60, 6, 8, 0, 0.3, d, 0.0, None, None),
        "rdst_swin_attn_fwd": lambda d: (p, 60, p, p, p, p, p, p, p, p, 180, p, 60, p, 60, p, p, z, 1, 16, 16, 60, 6, 8, 0, 0.3,
                                         d, None),
        "rdst_upsample2_fwd": lambda d: (p, 60, p, 60, 1, 8, 8, 60, d, None),
        "rdst_nchw_to_rows": lambda d: (p, p, 60, 1, 60, 8, 8, d, None),
        "rdst_u_conv": lambda d: (p, 64, 64, 0, None, 0, 0, p, None, None, 0, p, 64, 1, 16, 16, 16, 16, 64, 64, 3, 1, 0, d,
                                  None, None, None, None),
    }


@pytest.mark.parametrize("dtype", (-1, 3, 99))
def test_unknown_dtype_is_refused_before_any_launch(lib, dtype):
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    for name, args in _refusals(p).items():
        rc = getattr(lib, name)(*args(dtype))
        assert rc == _lib.EINVAL, (name, rc)
        assert b"bad dtype" in lib.rdst_last_error(), (name, lib.rdst_last_error())


if __name__ == "__main__" and "--record" in sys.argv:
    with open(TABLE, "w") as f:
        json.dump({name: answers(_lib.load(), name) for name in sorted(grids())}, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print("wrote", TABLE, "from", _lib.LIB_PATH)
