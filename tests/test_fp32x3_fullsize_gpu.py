"""fp32x3 parity AT THE SIZES bench.py RUNS its parity mode (BASELINE.json configs[1]: B 32 of 64x64, 131072 tokens, 2048
windows, 4096 row tiles): every fp32x3 op of the E1 training step straight through the C ABI, against float64.

The fp32x3 kernels (lin3x_mfma.hip, lnlin3x_mfma.hip, conv3x_mfma.hip, conv3x_wgrad.hip, conv_c1x.hip, the split forms of
wattn_mfma.hip / wattn_bwd_mfma.hip) run persistent grids capped for 256 CUs, slab reductions sized from those caps and DMA
row rings that wrap across images; at this size every workgroup loops many times, which the small cases of
test_fp32x3_gpu.py never make it do.

Reference: the same op in float64 with plain torch ON THE DEVICE (rocBLAS / torch kernels, nothing of this library): F.layer_norm,
F.gelu, F.linear; the 3x3 convolution as nine shifted float64 matmuls of the zero-padded image (`_conv64`: the same sum as
nn.Conv2d, with autograd of pad / slice / matmul for the gradients); window attention as the oracle's own
window_attention_core with the device as torch's default.  test_float64_device_reference_equals_cpu checks these device
references against float64 F.conv2d / the oracle on the CPU.

Gates on every output: finite; relative L2 over the tensor <= 3e-5 (the fp32x3 op gate); and tile-local relative L2
(tests/util.py local_rel: 32-token x 32-column tiles of Linear outputs and dX, one output-channel row of dW, one (image,
image row) of a convolution, one (window, head) of attention) under a gate picked from the measured worst (printed with -s).
A whole tile computed at bf16 precision gives ~1e-3 there (tests/test_gates.py).  Destinations are pre-filled with NaN, so
a tile that is never written cannot pass on memory left from an earlier correct run.

The parametrization tables below are the shape set of the E1 step; test_fp32x3_gpu.py::test_e1_fp32x3_shape_census fails when
the network calls one of these entry points at a shape missing here."""
import pytest
import torch
import torch.nn.functional as F

from oracle import rdst_oracle as O
from util import local_rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B_FULL, HW = 32, 64
M_FULL = B_FULL * HW * HW          # 131072 tokens
GLOBAL = 3e-5                      # relative L2 over the whole tensor (the fp32x3 op gate)
# tile-local gates: >= 10x the worst tile measured on an MI355X, <= 3e-4 (a bf16-precision tile sits at ~1e-3)
LOCAL_LIN = 1e-4                   # measured worst 6.8e-6 (dW rows), medians 2e-6 .. 4.5e-6
LOCAL_CONV = 1e-4                  # measured worst 5.2e-6 (dx of the head conv)
LOCAL_ATTN = 2e-4                  # measured worst 1.4e-5 (dqkv), medians 5e-6 .. 6e-6
LOCAL_DTABLE = 1e-4                # per head of d(table): measured worst 6.0e-6

# (K, N, ln, act, res, lin): lin = 0 is the LayerNorm alone (Wt = NULL, N = K)
LIN_CASES = [
    (60, 180, 1, 0, 0, 1), (90, 270, 1, 0, 0, 1), (120, 360, 1, 0, 0, 1),     # norm1 + qkv
    (60, 60, 0, 0, 1, 1), (90, 90, 0, 0, 1, 1), (120, 120, 0, 0, 1, 1),       # proj + shortcut
    (60, 120, 1, 0, 0, 1), (90, 180, 1, 0, 0, 1), (120, 240, 1, 0, 0, 1),     # norm2 + fc1
    (120, 60, 0, 1, 1, 1), (180, 90, 0, 1, 1, 1), (240, 120, 0, 1, 1, 1),     # GELU + fc2 + residual
    (60, 30, 1, 0, 0, 1), (90, 30, 1, 0, 0, 1), (120, 30, 1, 0, 0, 1),        # DenseSTLayer tails (LN + Linear(C, 30))
    (60, 60, 1, 0, 0, 0),                                                     # patch_embed.norm and the final norm
]
# (B, H, W, Cin, Cout, k, res, scale, r)
CONV_CASES = [
    (32, 64, 64, 60, 60, 3, 1, 1.0, 1),       # conv_after_body + global residual
    (32, 64, 64, 150, 60, 3, 1, 0.7, 1),      # RDB fusion conv * residual_scale + shortcut
    (32, 64, 64, 60, 240, 3, 0, 1.0, 2),      # upsampler stage 1 + PixelShuffle(2)
    (32, 128, 128, 60, 240, 3, 0, 1.0, 2),    # upsampler stage 2
    (32, 256, 256, 60, 1, 3, 0, 1.0, 1),      # conv_last 60 -> 1
    (32, 64, 64, 1, 60, 3, 0, 1.0, 1),        # head 1 -> 60 (conv_c1x.hip)
    (32, 64, 64, 1, 1, 1, 0, 1.0, 1),         # sub_mean (MeanShift, 1x1 on one channel)
    (32, 256, 256, 1, 1, 1, 0, 1.0, 1),       # add_mean
]
# (H, W, C, heads, ws, shift)
ATTN_CASES = [(HW, HW, C, 6, 8, s) for C in (60, 90, 120) for s in (0, 4)]


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(shape, g, scale=1.0):
    return scale * torch.randn(shape, generator=g, device=DEV, dtype=torch.float32)


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV, dtype=torch.float32)


def _ptr(t):
    return t.data_ptr() if t is not None else None


class _Report:
    """Collects (name, global rel L2, worst / median tile) per output; prints them, then gates them."""

    def __init__(self, title):
        self.title, self.rows = title, []

    def add(self, name, got, want, tiles, local, glob=GLOBAL):
        finite = bool(torch.isfinite(got).all())
        want = want.double()
        g = ((got.double() - want).norm() / want.norm().clamp_min(1e-300)).item() if finite else float("inf")
        worst, med, idx = local_rel(got, want, tiles) if (tiles and finite) else (g, g, ())
        local = glob if local is None else local
        self.rows.append((name, finite, g, worst, med, idx, local, glob))

    def check(self):
        print(f"\n{self.title}: " + "  ".join(f"{n} {g:.1e} [{w:.1e}/{m:.1e}]" for n, _, g, w, m, _, _, _ in self.rows))
        for n, finite, g, w, m, idx, local, glob in self.rows:
            assert finite, f"{self.title}: {n} has non-finite values (a tile never written?)"
            assert g <= glob, f"{self.title}: {n} rel L2 {g:.2e} > {glob:.0e}"
            assert w <= local, f"{self.title}: {n} worst tile {w:.2e} at {idx} (median {m:.2e}) > {local:.0e}"


# ------------------------------------------------------------------------------------------------------------------
# float64 references on the device
# ------------------------------------------------------------------------------------------------------------------
def _conv64(x, w, b, r=1, scale=1.0, res=None):
    """k x k convolution (stride 1, zero padding k // 2) of token-major x (B, H, W, Cin) -> (B, H*r, W*r, Cout / r^2):
    sum over the k*k taps of the shifted padded image times that tap's (Cout, Cin) weight, + bias, PixelShuffle(r)
    (nn.PixelShuffle's channel order: c*r*r + i*r + j), * scale, + res."""
    B, H, W, _ = x.shape
    k = w.shape[-1]
    p = k // 2
    xp = F.pad(x, (0, 0, p, p, p, p))
    y = b
    for ky in range(k):
        for kx in range(k):
            y = y + xp[:, ky:ky + H, kx:kx + W, :] @ w[:, :, ky, kx].t()
    if r > 1:
        c = y.shape[-1] // (r * r)
        y = y.view(B, H, W, c, r, r).permute(0, 1, 4, 2, 5, 3).reshape(B, H * r, W * r, c)
    y = y * scale
    return y + res if res is not None else y


def _attn64(qkv, table, heads, ws, shift, scale):
    """The oracle's window attention (oracle/rdst_oracle.py, pinned to swin_transformer_sr.py:110-141) on qkv's device:
    its index and mask tensors are made with torch's default device."""
    with torch.device(qkv.device):
        return O.window_attention_core(qkv, table, heads, ws, shift, scale)


def test_float64_device_reference_equals_cpu():
    """The device float64 references of this module against float64 on the CPU on small cases: the tap-sum convolution (with
    PixelShuffle, scale and residual) against F.conv2d / F.pixel_shuffle, forward and gradients; the attention against the
    oracle on the CPU, forward and gradients."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 16, 24, 60, generator=g, dtype=torch.float64)
    w = torch.randn(240, 60, 3, 3, generator=g, dtype=torch.float64) / 23.0
    b = torch.randn(240, generator=g, dtype=torch.float64)
    res = torch.randn(2, 32, 48, 60, generator=g, dtype=torch.float64)
    gy = torch.randn(2, 32, 48, 60, generator=g, dtype=torch.float64)
    xc, wc, bc = (t.clone().requires_grad_(True) for t in (x, w, b))
    yc = F.pixel_shuffle(F.conv2d(xc.permute(0, 3, 1, 2), wc, bc, padding=1), 2).permute(0, 2, 3, 1) * 0.7 + res
    yc.backward(gy)
    xd, wd, bd = (t.to(DEV).requires_grad_(True) for t in (x, w, b))
    yd = _conv64(xd, wd, bd, r=2, scale=0.7, res=res.to(DEV))
    yd.backward(gy.to(DEV))
    for got, want in ((yd, yc), (xd.grad, xc.grad), (wd.grad, wc.grad), (bd.grad, bc.grad)):
        assert (got.detach().cpu() - want.detach()).abs().max().item() <= 1e-12 * max(want.abs().max().item(), 1.0)

    qkv = torch.randn(2, 16, 24, 270, generator=g, dtype=torch.float64)
    table = 0.5 * torch.randn(225, 6, generator=g, dtype=torch.float64)
    gout = torch.randn(2, 16, 24, 90, generator=g, dtype=torch.float64)
    for shift in (0, 4):
        qc, tc = qkv.clone().requires_grad_(True), table.clone().requires_grad_(True)
        oc = O.window_attention_core(qc, tc, 6, 8, shift, 15 ** -0.5)
        oc.backward(gout)
        qd, td = qkv.to(DEV).requires_grad_(True), table.to(DEV).requires_grad_(True)
        od = _attn64(qd, td, 6, 8, shift, 15 ** -0.5)
        od.backward(gout.to(DEV))
        for got, want in ((od, oc), (qd.grad, qc.grad), (td.grad, tc.grad)):
            assert (got.detach().cpu() - want.detach()).abs().max().item() <= 1e-12 * max(want.abs().max().item(), 1.0)


# ------------------------------------------------------------------------------------------------------------------
# Linear: rdst_ln_linear_fwd, then the one-pass backward rdst_ln_linear_bwd2 with both dX addends, at M = 131072.  fc2 (GELU
# on the way in) never takes a second addend in the network and rdst_ln_linear_bwd2 refuses one there (RDST_ENOTSUP, nothing
# launched: include/rdst_hip.h); it and the LayerNorm alone run rdst_ln_linear_bwd with one addend, as the network calls them.
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,ln,act,res,lin", LIN_CASES)
def test_ln_linear_fp32x3_bench_size_vs_float64(K, N, ln, act, res, lin):
    from rdst_amd import _lib
    lib = _lib.load()
    M = M_FULL
    g = _gen(1000 + 7 * K + N)
    x = _randn((M, K), g)
    w, b = (_randn((N, K), g, K ** -0.5), _randn((N,), g, 0.1)) if lin else (None, None)
    lw, lb = (1 + _randn((K,), g, 0.1), _randn((K,), g, 0.1)) if ln else (None, None)
    r = _randn((M, N), g) if res else None
    gy = _randn((M, N), g)
    a1 = _randn((M, K), g)
    two = lin and act == 0                  # both dX addends: rdst_ln_linear_bwd2
    a2 = _randn((M, K), g) if two else None

    # float64 reference
    x64 = x.double().requires_grad_(True)
    p64 = {k: t.double().requires_grad_(True) for k, t in (("w", w), ("b", b), ("lw", lw), ("lb", lb)) if t is not None}
    h = F.layer_norm(x64, (K,), p64["lw"], p64["lb"], 1e-5) if ln else x64
    h = F.gelu(h) if act == 1 else h
    y64 = F.linear(h, p64["w"], p64["b"]) if lin else h
    y64 = y64 + r.double() if res else y64
    y64.backward(gy.double())
    dx64 = x64.grad + a1.double() + (a2.double() if two else 0)

    st = torch.cuda.current_stream().cuda_stream
    y = _nan(M, N)
    stats = _nan(M, 2) if ln else None
    nws = lib.rdst_ln_linear_fwd_workspace2(K, N, _lib.F32X3) if lin else 0
    wsf = torch.empty(max(nws, 16), dtype=torch.uint8, device=DEV)
    _lib.check(lib.rdst_ln_linear_fwd(x.data_ptr(), K, _ptr(lw), _ptr(lb), act, _ptr(w), _ptr(b), _ptr(r), N, y.data_ptr(), N,
                                      _ptr(stats), wsf.data_ptr() if lin else None, nws, M, K, N, 1.0, _lib.F32X3, st),
               "rdst_ln_linear_fwd")
    dx = _nan(M, K)
    dw, db = (_nan(N, K), _nan(N)) if lin else (None, None)
    dlw, dlb = (_nan(K), _nan(K)) if ln else (None, None)
    nb = lib.rdst_ln_linear_bwd_workspace(M, K, N)
    wsb = torch.empty(nb, dtype=torch.uint8, device=DEV)
    if two:
        rc = lib.rdst_ln_linear_bwd2(x.data_ptr(), K, _ptr(lw), _ptr(lb), _ptr(stats), act, w.data_ptr(), gy.data_ptr(), N,
                                     dx.data_ptr(), K, a1.data_ptr(), K, dw.data_ptr(), db.data_ptr(), _ptr(dlw), _ptr(dlb),
                                     wsb.data_ptr(), nb, M, K, N, 1.0, _lib.F32X3, st, a2.data_ptr(), K)
        assert rc == 0, (rc, lib.rdst_last_error())    # the one-pass kernels take these E1 shapes (no RDST_ENOTSUP)
    else:
        _lib.check(lib.rdst_ln_linear_bwd(x.data_ptr(), K, _ptr(lw), _ptr(lb), _ptr(stats), act, _ptr(w), gy.data_ptr(), N,
                                          dx.data_ptr(), K, a1.data_ptr(), K, _ptr(dw), _ptr(db), _ptr(dlw), _ptr(dlb),
                                          wsb.data_ptr(), nb, M, K, N, 1.0, _lib.F32X3, st), "rdst_ln_linear_bwd")
    torch.cuda.synchronize()

    rep = _Report(f"ln_linear fp32x3 K={K} N={N} ln={ln} act={act} res={res}{'' if lin else ' (LayerNorm only)'} M={M}")
    tile = {0: 32, 1: 32}
    rep.add("y", y, y64.detach(), tile, LOCAL_LIN)
    rep.add("dx", dx, dx64, tile, LOCAL_LIN)
    if lin:
        rep.add("dW", dw, p64["w"].grad, {0: 1}, LOCAL_LIN)
        rep.add("db", db, p64["b"].grad, None, None)
    if ln:
        rep.add("dgamma", dlw, p64["lw"].grad, None, None)
        rep.add("dbeta", dlb, p64["lb"].grad, None, None)
        xs = x.double()
        ref = torch.stack([xs.mean(1), torch.rsqrt(xs.var(1, unbiased=False) + 1e-5)], 1)
        assert torch.isfinite(stats).all()
        assert (stats.double() - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()
    rep.check()


# ------------------------------------------------------------------------------------------------------------------
# Convolution: rdst_conv_fwd + rdst_conv_bwd (dX, dW, db) at B = 32
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,Cin,Cout,k,res,scale,r", CONV_CASES)
def test_conv_fp32x3_bench_size_vs_float64(B, H, W, Cin, Cout, k, res, scale, r):
    from rdst_amd import _lib
    lib = _lib.load()
    g = _gen(2000 + 3 * Cin + Cout + H)
    cy = Cout // (r * r)
    x = _randn((B, H, W, Cin), g)
    w = _randn((Cout, Cin, k, k), g, (Cin * k * k) ** -0.5)
    bias = _randn((Cout,), g, 0.1)
    rr = _randn((B, H * r, W * r, cy), g) if res else None
    gy = _randn((B, H * r, W * r, cy), g)

    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, bias))
    y64 = _conv64(x64, w64, b64, r, scale, rr.double() if res else None)
    y64.backward(gy.double())

    st = torch.cuda.current_stream().cuda_stream
    y = _nan(B, H * r, W * r, cy)
    nws = lib.rdst_conv_fwd_workspace2(Cin, Cout, k, _lib.F32X3)
    wsf = torch.empty(max(nws, 16), dtype=torch.uint8, device=DEV)
    _lib.check(lib.rdst_conv_fwd(x.data_ptr(), Cin, 0, w.data_ptr(), bias.data_ptr(), _ptr(rr), cy, y.data_ptr(), cy,
                                 wsf.data_ptr(), nws, B, H, W, Cin, Cout, k, scale, r, _lib.F32X3, st), "rdst_conv_fwd")
    dx, dw, db = _nan(B, H, W, Cin), _nan(Cout, Cin, k, k), _nan(Cout)
    nb = lib.rdst_conv_bwd_workspace(B, H, W, Cin, Cout, k)
    wsb = torch.empty(nb, dtype=torch.uint8, device=DEV)
    _lib.check(lib.rdst_conv_bwd(x.data_ptr(), Cin, 0, w.data_ptr(), gy.data_ptr(), cy, dx.data_ptr(), Cin, None, 0,
                                 dw.data_ptr(), db.data_ptr(), wsb.data_ptr(), nb, B, H, W, Cin, Cout, k, scale, r,
                                 _lib.F32X3, st), "rdst_conv_bwd")
    torch.cuda.synchronize()

    rep = _Report(f"conv fp32x3 {Cin}->{Cout} k{k} r={r} res={res} scale={scale} {B}x{H}x{W}")
    rep.add("y", y, y64.detach(), {0: 1, 1: 1}, LOCAL_CONV)
    rep.add("dx", dx, x64.grad, {0: 1, 1: 1}, LOCAL_CONV)
    rep.add("dW", dw, w64.grad, {0: 1}, LOCAL_CONV)
    rep.add("db", db, b64.grad, None, None)
    rep.check()


# ------------------------------------------------------------------------------------------------------------------
# Window attention (split forms of wattn_mfma.hip / wattn_bwd_mfma.hip): 2048 windows
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,C,heads,ws,shift", ATTN_CASES)
def test_wattn_fp32x3_bench_size_vs_float64(H, W, C, heads, ws, shift):
    from rdst_amd import _lib
    lib = _lib.load()
    B = B_FULL
    scale = (C // heads) ** -0.5
    g = _gen(3000 + C + shift)
    qkv = _randn((B, H, W, 3 * C), g)
    table = _randn(((2 * ws - 1) ** 2, heads), g, 0.5)
    gout = _randn((B, H, W, C), g)

    q64, t64 = qkv.double().requires_grad_(True), table.double().requires_grad_(True)
    o64 = _attn64(q64, t64, heads, ws, shift, scale)
    o64.backward(gout.double())

    st = torch.cuda.current_stream().cuda_stream
    out = _nan(B, H, W, C)
    _lib.check(lib.rdst_wattn_fwd(qkv.data_ptr(), 3 * C, table.data_ptr(), None, 0, out.data_ptr(), C, B, H, W, C, heads, ws,
                                  shift, scale, _lib.F32X3, st), "rdst_wattn_fwd")
    dqkv, dtab = _nan(B, H, W, 3 * C), _nan((2 * ws - 1) ** 2, heads)
    nb = lib.rdst_wattn_bwd_workspace(B, H, W, C, heads, ws)
    wsb = torch.empty(max(nb, 16), dtype=torch.uint8, device=DEV)
    _lib.check(lib.rdst_wattn_bwd(qkv.data_ptr(), 3 * C, table.data_ptr(), None, 0, gout.data_ptr(), C, dqkv.data_ptr(), 3 * C,
                                  dtab.data_ptr(), wsb.data_ptr(), nb, B, H, W, C, heads, ws, shift, scale, _lib.F32X3, st),
               "rdst_wattn_bwd")
    torch.cuda.synchronize()

    # blocks = (image, window row, window column, head) in the shifted frame the windows are cut in
    roll = (lambda t: torch.roll(t, shifts=(-shift, -shift), dims=(1, 2))) if shift else (lambda t: t)
    win = {0: 1, 1: ws, 2: ws, 3: C // heads}
    rep = _Report(f"wattn fp32x3 {B}x{H}x{W} C={C} shift={shift}")
    rep.add("out", roll(out), roll(o64.detach()), win, LOCAL_ATTN)
    rep.add("dqkv", roll(dqkv), roll(q64.grad), win, LOCAL_ATTN)      # (q | k | v, head) per window
    rep.add("dtable", dtab, t64.grad, {1: 1}, LOCAL_DTABLE)            # per head
    rep.check()
