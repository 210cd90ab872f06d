"""The helpers of test_partial_grads_gpu.py, checked without a GPU: the float64 reference against plain fp32 autograd written
out here, the wide layout and the guarded workspace against a flipped byte, and the mask tables against the lists they
must hold (a silently shrunk table would leave a dispatch branch untested with the suite green)."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from oracle import rdst_oracle as O
from util import (ACT_GELU, ACT_LEAKY02, ACT_NONE, CONV_MASKS, LIN_MASKS_LN, LIN_MASKS_PLAIN, LN_ONLY_MASKS, GuardedWorkspace,
                  Wide, conv_bwd_ref, linear_bwd_ref, ln_stats, rand)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)).item()


@pytest.mark.parametrize("M,K,N,ln,act,with_add", [
    (37, 60, 180, True, ACT_NONE, False),      # norm1 + qkv
    (37, 120, 60, False, ACT_GELU, True),      # fc2 through GELU, dX_add
    (20, 33, 17, False, ACT_LEAKY02, True),    # odd sizes through LeakyReLU, dX_add
    (37, 60, 60, False, ACT_NONE, False),      # proj
])
def test_linear_reference_vs_fp32_autograd(M, K, N, ln, act, with_add):
    x, gy, add = rand((M, K), 1), rand((M, N), 2), rand((M, K), 3)
    lw, lb = (1 + 0.1 * rand((K,), 4), 0.1 * rand((K,), 5)) if ln else (None, None)
    w, b = rand((N, K), 6, K ** -0.5), 0.1 * rand((N,), 7)
    keep = [t.clone() for t in (x, gy, add, w, b)]
    ref = linear_bwd_ref(x, lw, lb, w, b, gy, act, 0.7, add if with_add else None)
    # plain fp32 autograd, written out
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    lwr, lbr = (lw.clone().requires_grad_(True), lb.clone().requires_grad_(True)) if ln else (None, None)
    h = F.layer_norm(xr, (K,), lwr, lbr, 1e-5) if ln else (O.gelu(xr) if act == ACT_GELU else F.leaky_relu(xr, 0.2) if act else xr)
    (F.linear(h, wr, br) * 0.7).backward(gy)
    want_dx = xr.grad + add if with_add else xr.grad
    assert all(v is None or v.dtype == torch.float64 for v in ref.values())
    assert _rel(ref["dx"], want_dx) <= 1e-5 and _rel(ref["dw"], wr.grad) <= 1e-5 and _rel(ref["db"], br.grad) <= 1e-5
    if ln:
        assert _rel(ref["dlw"], lwr.grad) <= 1e-5 and _rel(ref["dlb"], lbr.grad) <= 1e-5
    else:
        assert ref["dlw"] is None and ref["dlb"] is None
    for a, b_ in zip(keep, (x, gy, add, w, b)):   # the inputs are shared between tests: left as they were
        assert torch.equal(a, b_) and not b_.requires_grad


def test_layernorm_only_reference_and_stats():
    M, K = 29, 60
    x, gy = rand((M, K), 11), rand((M, K), 12)
    lw, lb = 1 + 0.1 * rand((K,), 13), 0.1 * rand((K,), 14)
    ref = linear_bwd_ref(x, lw, lb, None, None, gy, ACT_NONE, 0.5)
    xr, lwr, lbr = (t.clone().requires_grad_(True) for t in (x, lw, lb))
    (F.layer_norm(xr, (K,), lwr, lbr, 1e-5) * 0.5).backward(gy)
    assert ref["dw"] is None and ref["db"] is None
    assert _rel(ref["dx"], xr.grad) <= 1e-5 and _rel(ref["dlw"], lwr.grad) <= 1e-5 and _rel(ref["dlb"], lbr.grad) <= 1e-5
    st = ln_stats(x)
    assert st.shape == (M, 2) and st.dtype == torch.float32
    xhat = (x - st[:, :1]) * st[:, 1:]
    assert (xhat * lw + lb - F.layer_norm(x, (K,), lw, lb, 1e-5)).abs().max().item() <= 1e-5


@pytest.mark.parametrize("B,H,W,Cin,Cout,k,act,r,with_add", [
    (2, 5, 6, 7, 12, 3, ACT_LEAKY02, 1, True),     # through the activation, dX_add
    (1, 4, 5, 6, 16, 3, ACT_NONE, 2, False),       # PixelShuffle(2)
    (1, 3, 4, 5, 18, 3, ACT_NONE, 3, True),        # PixelShuffle(3)
    (2, 4, 4, 1, 1, 1, ACT_NONE, 1, False),        # one channel in and out, 1x1
])
def test_conv_reference_vs_fp32_autograd(B, H, W, Cin, Cout, k, act, r, with_add):
    cy = Cout // (r * r)
    x, gy, add = rand((B, H, W, Cin), 21), rand((B, H * r, W * r, cy), 22), rand((B, H, W, Cin), 23)
    w, b = rand((Cout, Cin, k, k), 24, (Cin * k * k) ** -0.5), 0.1 * rand((Cout,), 25)
    ref = conv_bwd_ref(x, w, b, gy, act, 0.7, r, add if with_add else None)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    h = xr.permute(0, 3, 1, 2)
    h = F.conv2d(F.leaky_relu(h, 0.2) if act == ACT_LEAKY02 else h, wr, br, padding=k // 2)
    h = F.pixel_shuffle(h, r) if r > 1 else h
    (h.permute(0, 2, 3, 1) * 0.7).backward(gy)
    want_dx = xr.grad + add if with_add else xr.grad
    assert ref["dx"].shape == x.shape and ref["dx"].dtype == torch.float64
    assert _rel(ref["dx"], want_dx) <= 1e-5 and _rel(ref["dw"], wr.grad) <= 1e-5 and _rel(ref["db"], br.grad) <= 1e-5


def test_a_dropped_scale_or_addend_shows_in_the_reference():
    """out_scale != 1 and dX_add are there so that a kernel that drops either is far outside every gate."""
    x, gy, add = rand((16, 24), 31), rand((16, 12), 32), rand((16, 24), 33)
    w, b = rand((12, 24), 34, 24 ** -0.5), 0.1 * rand((12,), 35)
    with_all = linear_bwd_ref(x, None, None, w, b, gy, ACT_NONE, 0.7, add)
    no_scale = linear_bwd_ref(x, None, None, w, b, gy, ACT_NONE, 1.0, add)
    no_add = linear_bwd_ref(x, None, None, w, b, gy, ACT_NONE, 0.7)
    assert _rel(no_scale["dw"], with_all["dw"]) > 0.3 and _rel(no_scale["db"], with_all["db"]) > 0.3
    assert _rel(no_add["dx"], with_all["dx"]) > 0.3


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("slot", ["x", "dy", "dx", "add"])
@pytest.mark.parametrize("cols", [1, 33, 37, 60, 150])
def test_wide_layout_round_trips_and_detects_a_flipped_byte(cols, slot, dtype):
    rows = 7
    w = Wide(rows, cols, dtype, slot)
    elt = 2 if dtype == torch.bfloat16 else 4
    assert w.ld >= w.off + cols + 1 and w.off >= 1            # untouched columns on both sides
    assert w.view.data_ptr() == w.buf.data_ptr() + w.off * elt and w.view.stride(0) == w.ld
    for r in range(rows):                                      # rows 4-byte aligned, never 16-byte aligned
        a = (w.off + r * w.ld) * elt
        assert a % 4 == 0 and a % 16 != 0
    src = rand((rows, cols), 41).to(dtype)
    w.view.copy_(src)
    assert torch.equal(w.view, src) and w.intact()
    w.view.fill_(float("nan"))                                 # whatever the slice holds, the surroundings are intact
    assert w.intact()
    for col in (w.off - 1, w.off + cols, w.ld - 1, 0):
        v = Wide(rows, cols, dtype, slot)
        v.buf.view(torch.uint8).view(-1)[(3 * v.ld + col) * elt] ^= 1    # one bit of one byte outside the slice
        assert not v.intact()


def test_guarded_workspace_detects_a_flipped_sentinel_byte():
    g = GuardedWorkspace(1001)
    assert g.buf.numel() == 1001 + 2 * 4096 and g.ptr() == g.buf.data_ptr() + 4096
    assert g.intact()
    g.buf[4096:4096 + 1001] = 7                                # the scratch itself is the kernel's to write
    assert g.intact()
    assert bool((GuardedWorkspace(64).buf[4096:4096 + 64] == 0xFF).all())   # scratch starts as fp32 NaN
    for pos in (0, 4095, 4096 + 1001, 2 * 4096 + 1000):       # first / last byte of either sentinel
        h = GuardedWorkspace(1001)
        h.buf[pos] ^= 1
        assert not h.intact(), pos


def test_mask_tables_hold_every_mask_of_the_issue():
    want_ln = {(1, 1, 1, 1, 1), (1, 0, 0, 0, 0), (0, 1, 1, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (1, 1, 0, 1, 1),
               (1, 0, 0, 1, 1), (0, 0, 0, 1, 1), (1, 1, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 1), (1, 0, 1, 0, 0)}
    assert set(LIN_MASKS_LN.values()) == want_ln and len(LIN_MASKS_LN) == 12
    want_plain = {(1, 1, 1, 0, 0), (1, 0, 0, 0, 0), (0, 1, 1, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (1, 1, 0, 0, 0),
                  (1, 0, 1, 0, 0)}
    assert set(LIN_MASKS_PLAIN.values()) == want_plain and len(LIN_MASKS_PLAIN) == 7
    subsets = [s for s in itertools.product((0, 1), repeat=3) if any(s)]
    assert set(LN_ONLY_MASKS.values()) == {(a, 0, 0, b, c) for a, b, c in subsets} and len(LN_ONLY_MASKS) == 7
    assert set(CONV_MASKS.values()) == set(subsets) and len(CONV_MASKS) == 7
    for table in (LIN_MASKS_LN, LIN_MASKS_PLAIN, LN_ONLY_MASKS, CONV_MASKS):   # the names say what the masks are
        for name, m in table.items():
            fields = ("dx", "dw", "db", "dlw", "dlb") if len(m) == 5 else ("dx", "dw", "db")
            assert name == "all" or name.split("+") == [f for f, on in zip(fields, m) if on], (name, m)


def test_gpu_file_runs_every_mask_table_and_case_of_the_issue():
    """The case lists of the GPU file (importable without a GPU): every shape the issue names is there."""
    import test_partial_grads_gpu as G
    lin = {(293, 60, 180, True, ACT_NONE), (293, 60, 60, False, ACT_NONE), (293, 120, 60, False, ACT_GELU),
           (293, 60, 120, True, ACT_NONE), (293, 120, 30, True, ACT_NONE), (40, 60, 180, True, ACT_NONE),
           (293, 90, 270, True, ACT_NONE), (293, 200, 40, True, ACT_NONE), (64, 33, 17, False, ACT_LEAKY02)}
    assert lin <= set(G.LIN_CASES) and set(G.LN_ONLY_CASES) == {60, 90, 33}
    conv = {(2, 6, 32, 150, 60, 3, ACT_NONE, 1), (2, 6, 10, 150, 60, 3, ACT_LEAKY02, 1), (1, 4, 32, 60, 240, 3, ACT_NONE, 2),
            (1, 5, 12, 60, 240, 3, ACT_NONE, 2), (2, 9, 11, 60, 1, 3, ACT_NONE, 1), (2, 9, 7, 1, 60, 3, ACT_NONE, 1),
            (2, 6, 6, 37, 12, 1, ACT_LEAKY02, 1), (1, 6, 6, 48, 108, 3, ACT_NONE, 3), (2, 16, 25, 1, 1, 1, ACT_NONE, 1)}
    assert conv <= set(G.CONV_CASES)
    assert set(G.MODES) == {"f32", "bf16", "f32x3"}
    assert len(G.FREEZE) == 8 and G.FREEZE["fc_weights_composed"][3] is False
    assert G._add_modes("all", 1) == ("none", "alias", "separate") and G._add_modes("dx", 1) == ("none", "alias")
    assert G._add_modes("dw", 0) == ("none",)
