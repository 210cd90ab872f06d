"""Exact results: Linear (ops.ln_linear and rdst_ln_linear_bwd), the convolutions on rows (ops.conv_rows) and window
attention (ops.window_attention) on operands whose result is exact in every order of summation, in every type the kernel
passes it through - compared with ``torch.equal`` against the float64 reference of exact_reference.py.

The bf16 gates elsewhere in the suite are norms (relative L2 8e-3 ... 2e-2): they let a strip seam, a dropped tap, a lost
pixel of a weight gradient or one wrong bias-table entry through.  Here operands are small integers (R1: bf16-representable,
power-of-two scales), every absolute sum stays below 2^24 quanta (R2) and below 256 where a partial sum is stored as bf16
(R3), so a term that is dropped, repeated or misplaced changes the result by at least one quantum.  R1 - R3 are asserted on
the CPU before every launch (exact_reference.check_rules); nothing is skipped.

Where the covered kernels round or narrow (read from the code; DESIGN.md carries the same table):

  output epilogues, every family     (acc + bias) * s + residual in fp32, then ONE round-to-nearest-even to bf16
                                     (conv_mfma.hip:146-148; dX of the Linear backward: lnlin_mfma.hip:309-332, dX_add added in fp32)
  Linear dW / dbias, bf16, one pass  per-workgroup partial sums as bf16 "G4" slabs (reduce_batch.h; written at
                                     lnlin_mfma.hip:341-351 and lnlin3_mfma.hip:260 ff.), summed over workgroups in fp32
  conv dW / dbias, bf16, 32-pixel    accumulator dumps as bf16 pairs (conv3_wgrad.hip:191-198), summed in fp32 and scaled by s
  row slabs (conv3_wgrad_bf16)       in conv3_wgrad_reduce_kernel
  every other weight gradient        fp32 slabs (linear_mfma.hip lin_wgrad, conv_mfma.hip conv_wgrad_mfma, conv_c1.hip,
                                     gemm_valu.h split-K, colsum): no narrowing
  fp32x3                             operands split into hi + lo bf16 terms, three products in fp32 (mfma.h Mma<float, true>);
                                     slabs fp32 (lnlin3x_mfma.hip:663, conv3x_wgrad.hip)

So in bf16 dW and dbias are asserted on the THINNED dY draw (R3: at most 256 per element; first and last pixel of every
image present), y and dX on the dense draw; in fp32 and fp32x3 everything is asserted on the dense draw, except where the
dense absolute sum of dW itself breaks R2 (fp32x3 with the hi + lo term on x at 33 x 6 x 256 pixels): dW then takes a
thinned draw bounded by 2^24 quanta.

Window attention runs with q = 0 and bias tables that make every softmax weight 0 or 2^-k (exact_reference.attn_table); the
leak of exp(-100) is asserted below 1e-38 max|v|.  bf16: |O - exact| <= 1/2 ulp_bf16(exact) + 1e-30, either neighbour on a
tie (normalising by a reciprocal may move a tie), the same for dV from integer dO.  fp32 and fp32x3: exact (<= 1e-30), output
and dV, on every route ops.window_attention takes - all of them form P from the row maximum and sum: wattn16_f32.hip:144-150
and :419 (window 16), wattn_mfma.hip:250-258 and wattn_bwd_mfma.hip:384-389, :471 (window 8), wattn_v0.hip (the scalar kernels:
window 4, 3 heads, head dim 8 at window 16).  The scalar backward used to keep max + logf(sum) and form P = expf(s - lse): a
probe-table row without a partner (every logit -100) then came back 2^-18 relative off (measured 3.8e-6 at window 16, 9.5e-7
at window 8: the rounding of a log-sum-exp near -95), beyond the 2^-20 sum_i P_ij |dO_i| that a stored log-sum-exp is allowed
here; it now keeps the maximum and 1 / sum like the forward.  The only stored log-sum-exp left is that of the bf16 window-16
kernels (wattn16_mfma.hip:191, :429; rdst_wattn_fwd_lse / rdst_wattn_bwd_lse), which ops.window_attention does not call:
test_window16_lse_entry_exact runs them through the C entry points under the bf16 rule (1/2 ulp), so no case needed the
2^-20 bound.  dq, dk and d(table) are not asserted.
"""
import functools

import pytest
import torch

import exact_reference as E
from util import GuardedWorkspace, Wide

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16, "f32x3": torch.float32}
PAD = 8          # columns on either side of a wide input slice
FILL = 3.0       # what they hold


def _scope(mode):
    from rdst_amd import ops
    return ops.compute_scope({"f32": ops.F32, "f32x3": ops.F32X3, "bf16": None}[mode])


def _code(mode):
    from rdst_amd import _lib
    return {"f32": _lib.F32, "bf16": _lib.BF16, "f32x3": _lib.F32X3}[mode]


def _dev(t, dtype, grad=False, wide=False):
    """`t` on the device in `dtype`: compact, or the middle columns of a wider buffer.  Returns (leaf, buffer or None)."""
    if t is None:
        return None, None
    if not wide:
        return t.to(DEV).to(dtype).requires_grad_(grad), None
    buf = torch.full(t.shape[:-1] + (t.shape[-1] + 2 * PAD,), FILL, dtype=dtype, device=DEV)
    buf[..., PAD:-PAD] = t.to(DEV).to(dtype)
    return buf[..., PAD:-PAD].detach().requires_grad_(grad), buf


def _untouched(buf, t, dtype):
    if buf is None:
        return True
    return bool((buf[..., :PAD] == FILL).all()) and bool((buf[..., -PAD:] == FILL).all()) and \
        torch.equal(buf[..., PAD:-PAD].cpu(), t.to(dtype))


def _hilo_name(config):
    return {"int": None, "x_hilo": "x", "w_hilo": "w"}[config]


# ---------------------------------------------------------------------------------------------------------------------
# Linear through ops.ln_linear
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", E.MODES)
@pytest.mark.parametrize("M,K,N", E.LINEAR_SHAPES)
def test_linear_exact(M, K, N, mode):
    from rdst_amd import ops
    dt = DTYPE[mode]
    for config in E.CONFIGS[mode]:
        for vi, (bias, res, scale, act) in enumerate(E.LINEAR_VARIANTS):
            op = E.linear_operands(M, K, N, config, act, 1000 + 10 * vi)
            b = op["b"] if bias else None
            r = op["res"] if res else None
            for name, gy, rows, asserted in E.linear_draws(op, N, mode, config, 1000 + 10 * vi):
                ref = E.linear_ref(op["x"], op["w"], b, r, gy, None, act, scale)
                bounds = E.linear_abs(op["x"], op["w"], b, r, gy, None, config)
                E.check_rules({"x": op["x"], "w": op["w"], "b": b, "res": r, "dy": gy}, _hilo_name(config), scale, bounds,
                              asserted, mode)
                for wide in (False, True):
                    tag = f"ln_linear {mode} {config} ({M},{K},{N}) bias={bias} res={res} s={scale} act={act} dY={name} " \
                          f"{'wide' if wide else 'compact'}"
                    xg, xbuf = _dev(op["x"], dt, True, wide)
                    rg, rbuf = _dev(r, dt, False, wide)
                    wg, _ = _dev(op["w"], torch.float32, True)
                    bg, _ = _dev(b, torch.float32, True)
                    with _scope(mode):
                        y = ops.ln_linear(xg, None, None, wg, bg, in_act=act, residual=rg, out_scale=scale)
                    y.backward(gy.to(DEV).to(dt))
                    torch.cuda.synchronize()
                    got = {"y": y.detach(), "dx": xg.grad, "dw": wg.grad, "db": bg.grad if bias else None}
                    for k in asserted:
                        if got[k] is None:
                            continue
                        want = E.expect(ref[k], dt if k in ("y", "dx") else torch.float32)
                        E.assert_equal(got[k], want, ("token", "channel") if k != "dw" else ("out", "in"), f"{tag}: {k}")
                    if rows is not None:      # tokens the thinned dY leaves out get no gradient at all
                        idle = torch.ones(M, dtype=torch.bool)
                        idle[rows] = False
                        assert bool((xg.grad.cpu()[idle] == 0).all()), f"{tag}: dX is nonzero where dY is zero"
                    assert _untouched(xbuf, op["x"], dt) and _untouched(rbuf, r, dt), f"{tag}: an input buffer was written"


# ---------------------------------------------------------------------------------------------------------------------
# Linear backward through the C entry point: dX_add, column slices of wider buffers, the guarded workspace
# ---------------------------------------------------------------------------------------------------------------------
class _Slot:
    def __init__(self, t2d, dtype, slot, wide):
        rows, cols = t2d.shape
        self.w = Wide(rows, cols, dtype, slot, DEV) if wide else None
        if wide:
            self.w.view.copy_(t2d.to(DEV).to(dtype))
            self.t, self.ld = self.w.view, self.w.ld
        else:
            self.t, self.ld = t2d.to(DEV).to(dtype).contiguous(), cols
        self.ptr = self.t.data_ptr()

    def intact(self):
        return self.w is None or self.w.intact()


@pytest.mark.parametrize("mode", E.MODES)
@pytest.mark.parametrize("M,K,N", E.LINEAR_SHAPES)
def test_linear_bwd_entry_exact(M, K, N, mode):
    from rdst_amd import _lib
    lib = _lib.load()
    dt = DTYPE[mode]
    prev = lib.rdst_side_enable(0)
    try:
        for config in E.CONFIGS[mode]:
            for vi, (act, scale, with_add) in enumerate(E.LINEAR_BWD_VARIANTS):
                op = E.linear_operands(M, K, N, config, act, 2000 + 10 * vi)
                add = op["add"] if with_add else None
                wg = op["w"].to(DEV).contiguous()
                nb = lib.rdst_ln_linear_bwd_workspace(M, K, N)
                for name, gy, rows, asserted in E.linear_draws(op, N, mode, config, 2000 + 10 * vi):
                    asserted = [k for k in asserted if k != "y"]
                    ref = E.linear_ref(op["x"], op["w"], op["b"], None, gy, add, act, scale)
                    bounds = E.linear_abs(op["x"], op["w"], op["b"], None, gy, add, config)
                    E.check_rules({"x": op["x"], "w": op["w"], "dy": gy, "dx_add": add}, _hilo_name(config), scale, bounds,
                                  asserted, mode)
                    for wide in (False, True):
                        tag = f"rdst_ln_linear_bwd {mode} {config} ({M},{K},{N}) act={act} s={scale} dX_add={with_add} dY={name} " \
                              f"{'wide' if wide else 'compact'}"
                        xo, gyo = _Slot(op["x"], dt, "x", wide), _Slot(gy, dt, "dy", wide)
                        addo = _Slot(add, dt, "add", wide) if with_add else None
                        dxo = _Slot(torch.full((M, K), float("nan")), dt, "dx", wide)
                        dW = torch.full((N, K), float("nan"), device=DEV)
                        db = torch.full((N,), float("nan"), device=DEV)
                        wsp = GuardedWorkspace(nb, DEV)
                        rc = lib.rdst_ln_linear_bwd(xo.ptr, xo.ld, None, None, None, act, wg.data_ptr(), gyo.ptr, gyo.ld, dxo.ptr, dxo.ld,
                                                    addo.ptr if addo else None, addo.ld if addo else 0, dW.data_ptr(), db.data_ptr(),
                                                    None, None, wsp.ptr(), nb, M, K, N, scale, _code(mode),
                                                    torch.cuda.current_stream().cuda_stream)
                        torch.cuda.synchronize()
                        assert rc == 0, f"{tag}: refused, rc={rc} {lib.rdst_last_error().decode(errors='replace')}"
                        assert wsp.intact(), f"{tag}: a workspace sentinel was overwritten"
                        assert dxo.intact(), f"{tag}: columns outside the dX slice were overwritten"
                        assert xo.intact() and gyo.intact() and (addo is None or addo.intact()), f"{tag}: an input buffer was written"
                        got = {"dx": dxo.t, "dw": dW, "db": db}
                        for k in asserted:
                            want = E.expect(ref[k], dt if k == "dx" else torch.float32)
                            E.assert_equal(got[k], want, ("token", "channel") if k != "dw" else ("out", "in"), f"{tag}: {k}")
                        if rows is not None:      # a token with a zero dY row: exactly dX_add, or zero
                            idle = torch.ones(M, dtype=torch.bool)
                            idle[rows] = False
                            want = add[idle].to(dt) if with_add else torch.zeros(int(idle.sum()), K, dtype=dt)
                            assert torch.equal(dxo.t.cpu()[idle], want), f"{tag}: dX differs from dX_add where dY is zero"
    finally:
        lib.rdst_side_enable(prev)


# ---------------------------------------------------------------------------------------------------------------------
# convolutions through ops.conv_rows
# ---------------------------------------------------------------------------------------------------------------------
NAMES4 = ("image", "row", "column", "channel")
NAMESW = ("out", "in", "ky", "kx")


@functools.lru_cache(maxsize=2)
def _conv_dense(case, config):
    """Operands, the dense dY, the float64 reference and the absolute sums of one case: shared by the modes, read only."""
    B, H, W, Cin, Cout, k, act, res, scale, r = case
    op = E.conv_operands(B, H, W, Cin, Cout, k, act, r, config, 3000)
    rr = op["res"] if res else None
    gy = E.dense_gy(tuple(op["res"].shape), 3005)
    ref = E.conv_ref(op["x"], op["w"], op["b"], rr, gy, act, scale, r)
    bounds = E.conv_abs(op["x"], op["w"], op["b"], rr, gy, r, config)
    return op, rr, gy, ref, bounds


def _conv_run(op, rr, gy, case, mode, x_grad):
    from rdst_amd import ops
    B, H, W, Cin, Cout, k, act, res, scale, r = case
    dt = DTYPE[mode]
    xg, _ = _dev(op["x"], dt, x_grad)
    wg, _ = _dev(op["w"], torch.float32, True)
    bg, _ = _dev(op["b"], torch.float32, True)
    rg, _ = _dev(rr, dt)
    with _scope(mode):
        y = ops.conv_rows(xg, wg, bg, in_act=act, residual=rg, out_scale=scale, shuffle=r)
    y.backward(gy.to(DEV).to(dt))
    torch.cuda.synchronize()
    return {"y": y.detach(), "dx": xg.grad, "dw": wg.grad, "db": bg.grad}


def _conv_exact(case, mode, x_grad):
    B, H, W, Cin, Cout, k, act, res, scale, r = case
    dt = DTYPE[mode]
    for config in E.CONFIGS[mode]:
        qs = E.quanta(config)
        op, rr, gy, ref, bounds = _conv_dense(case, config)
        asserted, dense_w = E.conv_dense_asserted(mode, bounds, x_grad)
        tag = f"conv_rows {mode} {config} {case}"
        E.check_rules({"x": op["x"], "w": op["w"], "b": op["b"], "res": rr, "dy": gy}, _hilo_name(config), scale, bounds, asserted, mode)
        got = _conv_run(op, rr, gy, case, mode, x_grad)
        for k_ in asserted:
            want = E.expect(ref[k_], dt if k_ in ("y", "dx") else torch.float32)
            E.assert_equal(got[k_], want, NAMESW if k_ == "dw" else NAMES4 if k_ != "db" else ("out",), f"{tag} dense dY: {k_}")
        if dense_w:
            continue
        limit = E.conv_thin_limit(mode, config)
        for s in E.thin_seeds(B, H, W):
            gt, rows = E.conv_thin_gy(op["x"], Cout, k, r, 3100 + s, limit)
            tref = E.conv_wgrad_sparse(op["x"], gt, rows, Cout, k, scale, r)
            tb = E.conv_wgrad_sparse(op["x"].abs(), gt.abs(), rows, Cout, k, 1.0, r)
            tbounds = {k_: v.max().item() / qs[k_] for k_, v in tb.items()}
            E.check_rules({"dy": gt}, None, scale, tbounds, ("dw", "db"), mode)
            got = _conv_run(op, rr, gt, case, mode, x_grad)
            for k_ in ("dw", "db"):
                E.assert_equal(got[k_], E.expect(tref[k_], torch.float32), NAMESW if k_ == "dw" else ("out",),
                               f"{tag} thinned dY (seed {s}, {len(rows)} pixels): {k_}")


@pytest.mark.parametrize("mode", E.MODES)
@pytest.mark.parametrize("case", E.CONV_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_conv_exact(case, mode):
    _conv_exact(case, mode, True)


@pytest.mark.parametrize("mode", E.MODES)
@pytest.mark.parametrize("B,H,W,Cout,scale", E.HEAD_CONV_CASES)
def test_head_conv_exact(B, H, W, Cout, scale, mode):
    """The head conv on a single-channel image that asks for no input gradient (conv_c1.hip / conv_c1x.hip in mirrored form)."""
    _conv_exact((B, H, W, 1, Cout, 3, 0, False, scale, 1), mode, False)


# ---------------------------------------------------------------------------------------------------------------------
# window attention with hard weights
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", E.MODES)
@pytest.mark.parametrize("B,H,W,C,heads,ws,shift,kind", E.ATTN_RUNS)
def test_window_attention_exact(B, H, W, C, heads, ws, shift, kind, mode):
    from rdst_amd import ops
    dt = DTYPE[mode]
    c = E.attn_case(B, H, W, C, heads, ws, shift, kind)
    tag = f"window_attention {mode} {(B, H, W, C, heads, ws, shift)} table={kind}"
    # preconditions, on the CPU: operands bf16-exact, every weight 0 or 2^-k, the leak of exp(-100) negligible
    assert E.is_bf16(c["qkv"]) and E.is_bf16(c["dO"]) and E.is_bf16(c["table"])
    assert c["dev"] <= 1e-30, f"{tag}: a softmax weight is {c['dev']:.3e} away from 0 / 2^-k"
    vmax = c["qkv"][..., 2 * C:].abs().max().item()
    assert (c["soft_o"] - c["o"]).abs().max().item() <= 1e-38 * vmax, f"{tag}: the leak of exp(-100)"
    assert c["abs_o"].max().item() < E.LIMIT_F32 and c["abs_dv"].max().item() < E.LIMIT_F32

    q = c["qkv"].to(DEV).to(dt).requires_grad_(True)
    t = c["table"].to(DEV).requires_grad_(True)
    with _scope(mode):
        o = ops.window_attention(q, t, H, W, heads, ws, shift, 0.25)
    o.backward(c["dO"].to(DEV).to(dt))
    torch.cuda.synchronize()
    dv = q.grad[..., 2 * C:]
    if mode == "bf16":
        tol_o, tol_dv = E.bf16_half_ulp(c["o"]) + 1e-30, E.bf16_half_ulp(c["dv"]) + 1e-30
    else:
        tol_o = tol_dv = 1e-30
    E.assert_within(o, c["o"], tol_o, NAMES4, f"{tag}: O")
    E.assert_within(dv, c["dv"], tol_dv, NAMES4, f"{tag}: dV")


@pytest.mark.parametrize("B,H,W,C,heads,ws,shift,kind", [r for r in E.ATTN_RUNS if r[5] == 16 and r[3] // r[4] in (10, 15, 20)])
def test_window16_lse_entry_exact(B, H, W, C, heads, ws, shift, kind):
    """rdst_wattn_fwd_lse / rdst_wattn_bwd_lse (bf16, window 16: the forward's row statistics kept for the backward), which
    ops.swin_block calls (head dims 10 / 15 / 20, the shapes they take): O and dV within half a bf16 ulp of the exact result."""
    from rdst_amd import _lib
    lib = _lib.load()
    c = E.attn_case(B, H, W, C, heads, ws, shift, kind)
    tag = f"rdst_wattn_*_lse {(B, H, W, C, heads, ws, shift)} table={kind}"
    assert c["dev"] <= 1e-30, f"{tag}: a softmax weight is {c['dev']:.3e} away from 0 / 2^-k"
    M = B * H * W
    qg, tg, gg = c["qkv"].to(DEV).bfloat16(), c["table"].to(DEV), c["dO"].to(DEV).bfloat16()
    st = torch.cuda.current_stream().cuda_stream
    out = torch.full((M, C), float("nan"), dtype=torch.bfloat16, device=DEV)
    nlse = torch.full((M, heads), float("nan"), device=DEV)
    _lib.check(lib.rdst_wattn_fwd_lse(qg.data_ptr(), 3 * C, tg.data_ptr(), out.data_ptr(), C, nlse.data_ptr(), B, H, W, C, heads, ws,
                                      shift, 0.25, _lib.BF16, st), "rdst_wattn_fwd_lse")
    nb = lib.rdst_wattn_bwd_workspace(B, H, W, C, heads, ws)
    dq = torch.full((M, 3 * C), float("nan"), dtype=torch.bfloat16, device=DEV)
    dtab = torch.full_like(tg, float("nan"))
    wsp = GuardedWorkspace(nb, DEV)
    _lib.check(lib.rdst_wattn_bwd_lse(qg.data_ptr(), 3 * C, tg.data_ptr(), gg.data_ptr(), C, out.data_ptr(), C, nlse.data_ptr(),
                                      dq.data_ptr(), 3 * C, dtab.data_ptr(), wsp.ptr(), nb, B, H, W, C, heads, ws, shift, 0.25,
                                      _lib.BF16, st), "rdst_wattn_bwd_lse")
    torch.cuda.synchronize()
    assert wsp.intact(), f"{tag}: a workspace sentinel was overwritten"
    E.assert_within(out.reshape(B, H, W, C), c["o"], E.bf16_half_ulp(c["o"]) + 1e-30, NAMES4, f"{tag}: O")
    E.assert_within(dq.reshape(B, H, W, 3 * C)[..., 2 * C:], c["dv"], E.bf16_half_ulp(c["dv"]) + 1e-30, NAMES4, f"{tag}: dV")
