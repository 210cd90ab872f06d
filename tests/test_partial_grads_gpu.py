"""Partial gradient requests: rdst_ln_linear_bwd, rdst_conv_bwd (through the C ABI, where the request mask IS the pattern of
NULL output pointers) and ops.swin_block (through autograd, with frozen parameters) against float64 autograd on the CPU.

The backward dispatch of csrc/linear.hip (bwd_t, ln_only_bwd) and csrc/conv.hip (bwd_impl) is chosen mostly by which
gradients are NOT wanted: the one-pass kernels run only when everything is requested, every other request goes to the
kernels below them (linear_wgrad_mfma, colsum, split-K gemm_valu + slab_reduce, linear_dgrad_ln_mfma + slab_reduce2,
linear_dgrad_mfma, ln_bwd_rows_kernel<KC>; conv3_*grad_*, conv_in1_wgrad_*, conv_*grad_mfma, plain_dy, gemm_valu).  Each
case below names the branch it is meant to reach, read from the code.

Every call runs in two layouts (compact; "wide": X, dY, dX, dX_add as column slices of wider buffers whose rows are 4-byte
but never 16-byte aligned), with every requested output pre-filled with NaN, the columns around a wide dX holding a bit
pattern and the workspace between two 4096-byte sentinels: all of them are checked after the call.

Gates (the project's own for the same op and mode): relative L2 per output 1e-4 (RDST_F32), 2e-2 (RDST_BF16), 3e-5
(RDST_F32X3); tile by tile (util.local_rel: 32-row blocks of dX of a Linear, image rows of dX of a conv, output-channel
rows of dW) twice that, 1e-4 for RDST_F32X3.  The swin block: 2e-4 (fp32, test_modules_gpu.py) and 2e-2 (bf16).

Worst values measured on an MI355X over every case, mask, layout and dX_add form (global relative L2 / tile-local):

    family            RDST_F32              RDST_BF16             RDST_F32X3
    Linear            4.0e-7 / 3.5e-7       2.4e-3 / 2.5e-3       4.1e-6 / 6.4e-6
    LayerNorm only    1.0e-7 / 6.4e-8       1.7e-3 / 1.8e-3       1.0e-7 / 6.4e-8    (no GEMM: fp32x3 = fp32)
    conv              1.9e-6 / 1.9e-6       2.4e-3 / 3.1e-3       4.4e-6 / 5.9e-6
    swin block        5.3e-7                6.7e-3                -

(bf16: the rounding of dX to bf16 alone is 2^-9 / sqrt(3) = 1.1e-3 relative; the fp32 conv figure is the single weight of the
one-channel 1x1 conv, a sum over 800 pixels.)  No mask was refused, every sentinel and every column outside a slice came back
intact.  Before the fix in bwd_t (csrc/linear.hip) the masks with d(gamma) / d(beta) and no dX behind a Linear came back
non-finite: ln_bwd_rows_kernel read a dA that only the dX branch computed (here the workspace starts as NaN).
"""
import functools

import pytest
import torch

from oracle import rdst_oracle as O
from rdst_amd import _lib
from util import (ACT_GELU, ACT_LEAKY02, ACT_NONE, CONV_MASKS, LIN_MASKS_LN, LIN_MASKS_PLAIN, LN_ONLY_MASKS, GuardedWorkspace,
                  Wide, conv_bwd_ref, linear_bwd_ref, ln_stats, local_rel, rand)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# mode: (dtype code, row dtype, global gate, tile gate)
MODES = {
    "f32": (_lib.F32, torch.float32, 1e-4, 2e-4),
    "bf16": (_lib.BF16, torch.bfloat16, 2e-2, 4e-2),
    "f32x3": (_lib.F32X3, torch.float32, 3e-5, 1e-4),
}

LIN_CASES = [  # (M, K, N, ln, act): what the masks below the all-gradients one reach in bwd_t (csrc/linear.hip)
    # norm1 + qkv, 293 = 9 * 32 + 5 (ragged last tile).  dW / dbias: linear_wgrad_mfma on LN(x) (lin_wgrad_mfma_kernel, XF = 1) and
    # the MAP_LINEAR slab sum with a NULL `out` or `out2`; dX: linear_dgrad_ln_mfma + slab_reduce2 (d(gamma) / d(beta), either NULL);
    # d(gamma) / d(beta) without dX: linear_dgrad_mfma into the fp32 dA, then ln_bwd_rows_kernel<1> with dX == NULL.
    # all: linear_ln_bwd_fused_bf16 (bf16), linear_wgrad_ln_mfma + linear_dgrad_ln2_mfma (fp32), lnlin3x_bwd_f32 (fp32x3)
    (293, 60, 180, True, ACT_NONE),
    # proj.  No LayerNorm: `slabW` starts at the workspace's first byte.  linear_wgrad_mfma (XF = 0) + linear_dgrad_mfma with the
    # dX epilogue (dX_add read in the kernel); all (bf16): the plain form of linear_ln_bwd_fused_bf16
    (293, 60, 60, False, ACT_NONE),
    # fc2 read through GELU: linear_wgrad_mfma (XF = 2: GELU on the staged x), linear_dgrad_mfma times gelu'(x)
    (293, 120, 60, False, ACT_GELU),
    # norm2 + fc1: as the first case at N = 2 K
    (293, 60, 120, True, ACT_NONE),
    # dense tail: one column tile of N = 30 on K = 120 (four LayerNorm channel tiles in linear_dgrad_ln_mfma)
    (293, 120, 30, True, ACT_NONE),
    # N (K + 1) > M K: the scratch gate of the one-pass branch flips, so even the all-gradients mask takes
    # linear_wgrad_mfma + linear_dgrad_ln_mfma (G does not fit dA); 40 rows: one full and one ragged 32-row slab
    (40, 60, 180, True, ACT_NONE),
    # qkv at C = 90: fp32 weights of 270 x 90 are the widest a resident-weight data-gradient kernel may still hold (all gradients,
    # fp32: linear_dgrad_ln2_mfma whole, or as two halves of N where it refuses); partial masks: linear_dgrad_ln_mfma with three
    # LayerNorm channel tiles, and d(gamma) / d(beta) without dX: linear_dgrad_mfma -> dA -> ln_bwd_rows_kernel<2>
    (293, 90, 270, True, ACT_NONE),
    # (added) qkv at C = 120: 360 x 120 fp32 weights exceed the LDS: all gradients in RDST_F32 run linear_dgrad_ln2_mfma as two
    # halves of N, the second accumulating onto dX in place (with dX_add aliased to dX as well); partial masks in the fp32 modes:
    # 45 k-steps of 8 > 32, linear_dgrad_ln_mfma and linear_dgrad_mfma refuse: gemm_valu with the DaEp epilogue -> dA ->
    # ln_bwd_rows_kernel<2>
    (293, 120, 360, True, ACT_NONE),
    # K > 128: no fused branch at all.  linear_wgrad_mfma (KT = 7), linear_dgrad_mfma -> dA, ln_bwd_rows_kernel<4> + slab_reduce2
    (293, 200, 40, True, ACT_NONE),
    # odd sizes through LeakyReLU(0.2).  bf16: rows of 66 / 34 bytes are not dword multiples, every MFMA kernel declines:
    # colsum_launch (dbias), split-K gemm_valu + slab_reduce (dW), gemm_valu with the DxEp epilogue (dX, act', dX_add);
    # fp32: rows of 132 / 68 bytes, the MFMA kernels take them
    (64, 33, 17, False, ACT_LEAKY02),
    # (added) rows of N = 3 elements are under 16 bytes in every mode: the gemm_valu fallbacks of the fp32 modes too
    (64, 33, 3, False, ACT_LEAKY02),
    # (added) ... behind a LayerNorm with K > 128: gemm_valu on LinInT (wgrad), gemm_valu with the DaEp epilogue (dA),
    # ln_bwd_rows_kernel<4>
    (64, 200, 3, True, ACT_NONE),
]
LN_ONLY_CASES = [  # K = N, Wt == NULL: ln_only_bwd
    60,   # ln8_bwd_kernel (8 <= K <= 64, even): the last 8-channel chunk of a row overlaps its neighbour; dX == NULL in the kernel
    90,   # K > 64: scale_to_f32_kernel + ln_bwd_rows_kernel<2>
    33,   # odd K: ln8_ok refuses, scale_to_f32_kernel + ln_bwd_rows_kernel<1>
]
CONV_CASES = [  # (B, H, W, Cin, Cout, k, act, r, also): what bwd_impl (csrc/conv.hip) reaches
    # register-stationary kernels on 32-pixel row slabs, gated separately: conv3_dgrad_bf16 / conv3x_dgrad_f32 on dX,
    # conv3_wgrad_bf16 / conv3x_wgrad_f32 on dW || dbias (their reduce with dW or dbias NULL); RDST_F32: conv_wgrad_mfma (the
    # pipelined rows kernel) + conv_dgrad_mfma (launch_conv_rows)
    (2, 6, 32, 150, 60, 3, ACT_NONE, 1),
    # W % 32 != 0 and an input activation: the register-stationary kernels decline; pixel-tile conv_wgrad_mfma_kernel +
    # conv_wgrad_reduce_kernel (dW / dbias NULL), conv_dgrad_mfma (launch_conv) times leaky'(x)
    (2, 6, 10, 150, 60, 3, ACT_LEAKY02, 1),
    # 60 -> 240 + PixelShuffle(2), W % 32 == 0: conv3_*_bf16 / conv3x_* read the shuffled dY as it lies (compact: ld_dy == 60);
    # the wide layout (ld_dy != 60) makes the bf16 kernels decline: plain_dy (unshuffle2_*) + conv_*grad_mfma; RDST_F32: dgrad in 4 slices
    (1, 4, 32, 60, 240, 3, ACT_NONE, 2),
    # the same conv at W % 32 != 0: always plain_dy + the pixel-tile kernels (RDST_F32: dgrad in two slices of 120, in place)
    (1, 5, 12, 60, 240, 3, ACT_NONE, 2),
    # tail, one output channel: conv_c1_bwd_bf16 / conv_c1x_bwd_f32 (wgrad on `wst` + reduce + copies gated on dW || dbias,
    # dgrad gated on dX), slab at the END of the workspace
    (2, 9, 11, 60, 1, 3, ACT_NONE, 1),
    # head, one input channel: conv_in1_wgrad_bf16 / conv_in1x_wgrad_f32 only with !dX; with dX requested the call leaves them
    # for conv_wgrad_mfma / gemm_valu and the dgrad fallbacks
    (2, 9, 7, 1, 60, 3, ACT_NONE, 1),
    # 1x1 through LeakyReLU, Cin = 37 (odd: bf16 rows of 74 bytes, packs loaded element by element): conv_wgrad_mfma_kernel at
    # ks = 1 (one grid row) + conv_wgrad_reduce_kernel, conv_dgrad_mfma (launch_conv) times leaky'(x)
    (2, 6, 6, 37, 12, 1, ACT_LEAKY02, 1),
    # x3 shuffle: plain_dy through the generic unshuffle_kernel (r = 3)
    (1, 6, 6, 48, 108, 3, ACT_NONE, 3),
    # one channel in and out, 1x1 (MeanShift): dX alone = conv_pw11_kernel / c1x_pw11_kernel (strided form in the wide
    # layout); any parameter gradient: conv_wgrad_mfma_kernel, and dX beside it on gemm_valu with ConvDxEp (Cout < 8:
    # conv_dgrad_mfma declines)
    (2, 16, 25, 1, 1, 1, ACT_NONE, 1),
    # (added) 5 x 3 x 4 = 60 accumulator tiles > 48: conv_wgrad_mfma declines in every mode: colsum_launch (ConvDyCol) for dbias,
    # split-K gemm_valu with ConvSlabEp + slab_reduce for dW; RDST_F32: conv_dgrad_mfma in two slices of 65 output channels
    (1, 4, 6, 100, 130, 3, ACT_NONE, 1),
]


def _round(t, dtype):
    return t.to(dtype).float() if dtype == torch.bfloat16 else t


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Operand:
    """An input matrix on the device, compact or as a slice of a wider buffer."""

    def __init__(self, t2d, dtype, slot, wide):
        rows, cols = t2d.shape
        if wide:
            self.w = Wide(rows, cols, dtype, slot, DEV)
            self.w.view.copy_(t2d.to(DEV).to(dtype))
            self.t, self.ld = self.w.view, self.w.ld
        else:
            self.w = None
            self.t, self.ld = t2d.to(DEV).to(dtype).contiguous(), cols
        self.ptr = self.t.data_ptr()

    def intact(self):
        return self.w is None or self.w.intact()


class _Checker:
    """Collects every miss of a test (so one run names all of them) and the worst measured values."""

    def __init__(self, tol, tile_tol):
        self.tol, self.tile_tol, self.bad, self.worst = tol, tile_tol, [], {}

    def fail(self, tag, msg):
        self.bad.append(f"{tag}: {msg}")

    def _note(self, key, v):
        self.worst[key] = max(self.worst.get(key, 0.0), v)

    def compare(self, tag, name, got, want, tiles=None):
        got = got.detach().float().cpu()
        if not bool(torch.isfinite(got).all()):
            return self.fail(tag, f"{name} is not finite ({int((~torch.isfinite(got)).sum())} of {got.numel()} elements)")
        rel = ((got.double() - want).norm() / want.norm().clamp_min(1e-300)).item()
        self._note(name, rel)
        if rel > self.tol:
            self.fail(tag, f"{name} relative L2 {rel:.3e} > {self.tol:.1e}")
        if tiles is not None:
            worst, med, idx = local_rel(got, want, tiles)
            self._note(name + " tile", worst)
            if worst > self.tile_tol:
                self.fail(tag, f"{name} tile {idx} local {worst:.3e} (median {med:.3e}) > {self.tile_tol:.1e}")

    def report(self, what):
        print(f"\n{what}: worst " + "  ".join(f"{k} {v:.2e}" for k, v in sorted(self.worst.items())))
        assert not self.bad, f"{len(self.bad)} misses:\n" + "\n".join(self.bad)


def _side_off(lib):
    return lib.rdst_side_enable(0)


def _add_modes(mask_name, wants_dx):
    if not wants_dx:
        return ("none",)
    return ("none", "alias", "separate") if mask_name == "all" else ("none", "alias")


def _dx_buffers(add_mode, add2d, rows, cols, dtype, wide):
    """(dX tensor view, ld, dX_add ptr, ld_add, wide dX or None, wide add or None): dX pre-filled with NaN, or with
    dX_add where the two alias."""
    wadd = None
    if wide:
        wdx = Wide(rows, cols, dtype, "dx", DEV)
        dx, ld = wdx.view, wdx.ld
    else:
        wdx = None
        dx, ld = torch.empty((rows, cols), dtype=dtype, device=DEV), cols
    if add_mode == "alias":
        dx.copy_(add2d.to(DEV).to(dtype))
        return dx, ld, dx.data_ptr(), ld, wdx, None
    dx.fill_(float("nan"))
    if add_mode == "none":
        return dx, ld, None, 0, wdx, None
    op = _Operand(add2d, dtype, "add", wide)
    return dx, ld, op.ptr, op.ld, wdx, op


def _run_linear(M, K, N, ln, act, mode, masks, scale, ln_only=False):
    lib = _lib.load()
    code, dtype, tol, tile_tol = MODES[mode]
    x = _round(rand((M, K), 101), dtype)
    gy = _round(rand((M, N), 102), dtype)
    add = _round(rand((M, K), 103), dtype)
    lw, lb = (1 + 0.1 * rand((K,), 104), 0.1 * rand((K,), 105)) if ln else (None, None)
    w, b = (None, None) if ln_only else (rand((N, K), 106, K ** -0.5), 0.1 * rand((N,), 107))
    ref = linear_bwd_ref(x, lw, lb, w, b, gy, act, scale)
    ref_add = ref["dx"] + add.double()
    stats = ln_stats(x).to(DEV) if ln else None
    P = [t.to(DEV).contiguous() if t is not None else None for t in (lw, lb, w, b)]
    nb = lib.rdst_ln_linear_bwd_workspace(M, K, N)
    ck = _Checker(tol, tile_tol)
    prev = _side_off(lib)
    try:
        for wide in (False, True):
            xo, gyo = _Operand(x, dtype, "x", wide), _Operand(gy, dtype, "dy", wide)
            for mname, (mx, mw, mb, mlw, mlb) in masks.items():
                for add_mode in _add_modes(mname, mx):
                    tag = f"{mode} ({M},{K},{N}) {'wide' if wide else 'compact'} mask={mname} dX_add={add_mode}"
                    dx, ld_dx, addp, ld_add, wdx, addo = (None, K, None, 0, None, None)
                    if mx:
                        dx, ld_dx, addp, ld_add, wdx, addo = _dx_buffers(add_mode, add, M, K, dtype, wide)
                    dW = _nan((N, K)) if mw else None
                    db = _nan((N,)) if mb else None
                    dlw = _nan((K,)) if mlw else None
                    dlb = _nan((K,)) if mlb else None
                    wsp = GuardedWorkspace(nb, DEV)
                    rc = lib.rdst_ln_linear_bwd(xo.ptr, xo.ld, _ptr(P[0]), _ptr(P[1]), _ptr(stats), act, _ptr(P[2]), gyo.ptr, gyo.ld,
                                                _ptr(dx), ld_dx, addp, ld_add, _ptr(dW), _ptr(db), _ptr(dlw), _ptr(dlb), wsp.ptr(), nb,
                                                M, K, N, scale, code, _stream())
                    torch.cuda.synchronize()
                    if rc != 0:
                        ck.fail(tag, f"refused: rc={rc} {lib.rdst_last_error().decode(errors='replace')}")
                        continue
                    if not wsp.intact():
                        ck.fail(tag, "a workspace sentinel was overwritten")
                    if wdx is not None and not wdx.intact():
                        ck.fail(tag, "columns outside the dX slice were overwritten")
                    if addo is not None and not addo.intact():
                        ck.fail(tag, "columns outside the dX_add slice were overwritten")
                    if mx:
                        ck.compare(tag, "dX", dx, ref["dx"] if add_mode == "none" else ref_add, {0: 32})
                    if mw:
                        ck.compare(tag, "dW", dW, ref["dw"], {0: 1})
                    if mb:
                        ck.compare(tag, "dbias", db, ref["db"])
                    if mlw:
                        ck.compare(tag, "dln_w", dlw, ref["dlw"])
                    if mlb:
                        ck.compare(tag, "dln_b", dlb, ref["dlb"])
            if not (xo.intact() and gyo.intact()):
                ck.fail(f"{mode} ({M},{K},{N}) wide", "an input buffer was written")
    finally:
        lib.rdst_side_enable(prev)
    ck.report(f"ln_linear_bwd {mode} M={M} K={K} N={N} ln={ln} act={act}")


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("M,K,N,ln,act", LIN_CASES)
def test_ln_linear_bwd_partial(M, K, N, ln, act, mode):
    _run_linear(M, K, N, ln, act, mode, LIN_MASKS_LN if ln else LIN_MASKS_PLAIN, 0.7)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("K", LN_ONLY_CASES)
def test_ln_only_bwd_partial(K, mode):
    _run_linear(293, K, K, True, ACT_NONE, mode, LN_ONLY_MASKS, 0.5, ln_only=True)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("B,H,W,Cin,Cout,k,act,r", CONV_CASES)
def test_conv_bwd_partial(B, H, W, Cin, Cout, k, act, r, mode):
    lib = _lib.load()
    code, dtype, tol, tile_tol = MODES[mode]
    cy = Cout // (r * r)
    P, Py = B * H * W, B * H * r * W * r
    x = _round(rand((B, H, W, Cin), 201), dtype)
    gy = _round(rand((B, H * r, W * r, cy), 202), dtype)
    add = _round(rand((B, H, W, Cin), 203), dtype)
    w = rand((Cout, Cin, k, k), 204, (Cin * k * k) ** -0.5)
    b = 0.1 * rand((Cout,), 205)
    scale = 0.7
    ref = conv_bwd_ref(x, w, b, gy, act, scale, r)
    ref_add = ref["dx"] + add.double()
    wg = w.to(DEV).contiguous()
    nb = lib.rdst_conv_bwd_workspace(B, H, W, Cin, Cout, k)
    ck = _Checker(tol, tile_tol)
    prev = _side_off(lib)
    try:
        for wide in (False, True):
            xo, gyo = _Operand(x.reshape(P, Cin), dtype, "x", wide), _Operand(gy.reshape(Py, cy), dtype, "dy", wide)
            for mname, (mx, mw, mb) in CONV_MASKS.items():
                for add_mode in _add_modes("all" if (mx and mw and mb) else mname, mx):
                    tag = f"{mode} {(B, H, W, Cin, Cout, k, r)} {'wide' if wide else 'compact'} mask={mname} dX_add={add_mode}"
                    dx, ld_dx, addp, ld_add, wdx, addo = (None, Cin, None, 0, None, None)
                    if mx:
                        dx, ld_dx, addp, ld_add, wdx, addo = _dx_buffers(add_mode, add.reshape(P, Cin), P, Cin, dtype, wide)
                    dW = _nan((Cout, Cin, k, k)) if mw else None
                    db = _nan((Cout,)) if mb else None
                    wsp = GuardedWorkspace(nb, DEV)
                    rc = lib.rdst_conv_bwd(xo.ptr, xo.ld, act, wg.data_ptr(), gyo.ptr, gyo.ld, _ptr(dx), ld_dx, addp, ld_add, _ptr(dW),
                                           _ptr(db), wsp.ptr(), nb, B, H, W, Cin, Cout, k, scale, r, code, _stream())
                    torch.cuda.synchronize()
                    if rc != 0:
                        ck.fail(tag, f"refused: rc={rc} {lib.rdst_last_error().decode(errors='replace')}")
                        continue
                    if not wsp.intact():
                        ck.fail(tag, "a workspace sentinel was overwritten")
                    if wdx is not None and not wdx.intact():
                        ck.fail(tag, "columns outside the dX slice were overwritten")
                    if addo is not None and not addo.intact():
                        ck.fail(tag, "columns outside the dX_add slice were overwritten")
                    if mx:
                        want = ref["dx"] if add_mode == "none" else ref_add
                        ck.compare(tag, "dX", dx.reshape(B, H, W, Cin), want, {0: 1, 1: 1})
                    if mw:
                        ck.compare(tag, "dW", dW, ref["dw"], {0: 1})
                    if mb:
                        ck.compare(tag, "dbias", db, ref["db"])
            if not (xo.intact() and gyo.intact()):
                ck.fail(f"{mode} wide", "an input buffer was written")
    finally:
        lib.rdst_side_enable(prev)
    ck.report(f"conv_bwd {mode} {(B, H, W, Cin, Cout, k, act, r)}")


# ---------------------------------------------------------------------------------------------------------------------
# ops.swin_block as autograd sees it: the GPU twins of the frozen-parameter scenarios of test_ops_trace.py
# ---------------------------------------------------------------------------------------------------------------------
BLK = dict(C=60, heads=6, ws=8, B=2, H=16, W=16, hid=120)
NAMES = ["norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.relative_position_bias_table",
         "attn.proj.weight", "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias",
         "mlp.fc2.weight", "mlp.fc2.bias"]
ALL_BUT_X = tuple(NAMES)
# name: (frozen parameters, parameters that are None, x requires grad, ops.MLP_FUSED)
FREEZE = {
    "table": (("attn.relative_position_bias_table",), (), True, None),
    "fc_weights": (("mlp.fc1.weight", "mlp.fc2.weight"), (), True, None),             # scratch destinations of the fused Mlp backward
    "fc_weights_composed": (("mlp.fc1.weight", "mlp.fc2.weight"), (), True, False),   # the composed path with NULLs
    "norm1": (("norm1.weight", "norm1.bias"), (), True, None),
    "qkv_weight": (("attn.qkv.weight",), (), True, None),                             # ... with a trainable qkv.bias
    "no_bias": ((), ("attn.qkv.bias", "attn.proj.bias"), True, None),
    "x_frozen": ((), (), False, None),
    "only_x": (ALL_BUT_X, (), True, None),
}


def _block_params():
    C, heads, ws, hid = BLK["C"], BLK["heads"], BLK["ws"], BLK["hid"]
    return {
        "norm1.weight": 1 + 0.1 * rand((C,), 301), "norm1.bias": 0.1 * rand((C,), 302),
        "attn.qkv.weight": rand((3 * C, C), 303, C ** -0.5), "attn.qkv.bias": 0.1 * rand((3 * C,), 304),
        "attn.relative_position_bias_table": 0.5 * rand(((2 * ws - 1) ** 2, heads), 305),
        "attn.proj.weight": rand((C, C), 306, C ** -0.5), "attn.proj.bias": 0.1 * rand((C,), 307),
        "norm2.weight": 1 + 0.1 * rand((C,), 308), "norm2.bias": 0.1 * rand((C,), 309),
        "mlp.fc1.weight": rand((hid, C), 310, C ** -0.5), "mlp.fc1.bias": 0.1 * rand((hid,), 311),
        "mlp.fc2.weight": rand((C, hid), 312, hid ** -0.5), "mlp.fc2.bias": 0.1 * rand((C,), 313),
    }


def _block_io(bf16):
    B, H, W, C = BLK["B"], BLK["H"], BLK["W"], BLK["C"]
    x, gy = rand((B, H * W, C), 320), rand((B, H * W, C), 321)
    return (x.bfloat16().float(), gy.bfloat16().float()) if bf16 else (x, gy)


@functools.lru_cache(maxsize=None)
def _block_ref(bf16, shift, no_bias):
    """Every gradient of the block in float64 (oracle.rdst_oracle.swin_block): shared by the freeze patterns, read only."""
    x, gy = _block_io(bf16)
    sd = {}
    for k, v in _block_params().items():
        none = no_bias and k in ("attn.qkv.bias", "attn.proj.bias")
        sd["p." + k] = None if none else v.double().requires_grad_(True)
    xr = x.double().requires_grad_(True)
    y = O.swin_block(xr, (BLK["H"], BLK["W"]), sd, "p.", BLK["heads"], BLK["ws"], shift)
    y.backward(gy.double())
    out = {k[2:]: (None if v is None else v.grad) for k, v in sd.items()}
    out["x"] = xr.grad
    return out


@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("pattern", list(FREEZE))
@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_swin_block_partial(mode, pattern, shift):
    from rdst_amd import ops
    frozen, none, x_grad, mlp_fused = FREEZE[pattern]
    bf16 = mode == "bf16"
    tol = 2e-2 if bf16 else 2e-4
    ref = _block_ref(bf16, shift, bool(none))
    x, gy = _block_io(bf16)
    dt = torch.bfloat16 if bf16 else torch.float32
    prm = {}
    for k, v in _block_params().items():
        prm[k] = None if k in none else v.to(DEV).requires_grad_(k not in frozen)
    xg = x.to(DEV).to(dt).requires_grad_(x_grad)
    keep = ops.MLP_FUSED
    try:
        if mlp_fused is not None:
            ops.MLP_FUSED = mlp_fused
        y = ops.swin_block(xg, *[prm[k] for k in NAMES], BLK["H"], BLK["W"], BLK["heads"], BLK["ws"], shift,
                           (BLK["C"] // BLK["heads"]) ** -0.5)
        y.backward(gy.to(DEV).to(dt))
        torch.cuda.synchronize()
    finally:
        ops.MLP_FUSED = keep
    ck = _Checker(tol, None)
    tag = f"{mode} {pattern} shift={shift}"
    if x_grad:
        ck.compare(tag, "x", xg.grad, ref["x"])
    else:
        assert xg.grad is None
    for k in NAMES:
        if prm[k] is None:
            continue
        if k in frozen:
            assert prm[k].grad is None, f"{tag}: frozen {k} got a gradient"
        else:
            assert prm[k].grad is not None, f"{tag}: {k} got no gradient"
            ck.compare(tag, k, prm[k].grad, ref[k])
    ck.report(f"swin_block {tag}")
