"""Exact results behind a LayerNorm, a GELU and through the fused Mlp: ops.ln_linear and rdst_ln_linear_bwd with ln_w / ln_b /
stats, the GELU Linear (fc2 of every composed Mlp), rdst_mlp_fwd on its three routes and rdst_mlp_bwd - on the hard operands of
exact_ln_reference.py, compared with ``torch.equal`` against its float64 hard evaluation.  test_exact_gpu.py holds the GEMMs
without a LayerNorm.  A relative-L2 gate sees a slip confined to one token or one tile less and less as the token count grows
(test_exact_ln_host.py has the figures: the gated tests of test_mlp_gpu.py do see most such slips at their 1189 tokens); this
comparison does not depend on the size.

Where these kernels round or narrow (read from the code and measured; DESIGN.md section 2 carries the table with the lines):

  row statistics            sum / (float)K (row_stats_kernel) or sum * fl(1 / K) (every other kernel); 1 / sqrtf (linear_mfma.hip,
                            mlp_mfma.hip) or rsqrtf (lin3_mfma.hip, mlp3_mfma.hip, lin3x_mfma.hip); var * invK + eps is contracted
                            into one fma, which makes rstd of s = 8 one ulp short of 1/8 at K = 60, 90, 120: the scales are drawn
                            from those that pass a float32 emulation of every formula (16 .. 128 there)
  x-hat, bf16               narrowed to bf16, i.e. to +-1 exactly, in the one-pass backward kernels (mlp_mfma.hip, lnlin_mfma.hip,
                            lnlin3_mfma.hip); kept in fp32 by the composed backward (linear_mfma.hip:920, :944): sigma (1 - eps / (2 s^2))
                            at s = 1, 2; NOT formed at all in the bf16 forwards, which work on the raw rows and apply
                            h = fma(rstd, acc, fma(-rstd mean, S, b')) in fp32 (lin3_mfma.hip, mlp3_mfma.hip, mlp_mfma.hip forward)
  GELU, Linear              gelu_erf / gelu_erf_grad (fp32), gelu_fast / gelu_grad_fast (bf16, fp32x3) in fp32; bf16 narrows the
                            product as an MFMA operand
  GELU, fused Mlp           the fp16 table (forward of mlp3_mfma.hip, backward of mlp_mfma.hip), gelu_pair (forward of mlp_mfma.hip);
                            h GELU and dH GELU' narrowed to bf16
  weight-gradient slabs     bf16 G4 groups in the one-pass Linear backward AND in rdst_mlp_bwd (mlp_mfma.hip:492-507): R3 applies
                            to G1 = dH'^T x-hat, db1, dW2 and db2, so they are asserted on the thinned dY draw
  dW1 = gamma G + beta db^T, d(gamma), d(beta)   fp32, in the LayerNorm finish (reduce_batch.hip:109-138) from the summed G

The Linear cases run at out_scale 1 (what the Swin blocks pass) and 1/2.  rdst_ln_linear_bwd hands a bf16 call with everything
requested to the one-pass kernels (lnlin_mfma.hip, lnlin3_mfma.hip) only at out_scale 1 and with room for G in its scratch,
N (K + 1) <= M K (exact_ln_reference.ln_onepass); every other call goes to the composed backward of linear_mfma.hip.  Each width
therefore has a small shape and one with enough tokens.

Asserted exactly: fp32 and fp32x3 - everything but dX behind a LayerNorm; bf16 - every parameter gradient of the one-pass route on
the thinned draw, s = 1, 2 rows included (a fallback there fails the test); of the composed route on the thinned draw over rows
of s >= 8, and within ln_wgrad_tol (about 1e-5 of the absolute sum) with the s = 1, 2 rows; everything of the GELU Linear; y of
the raw-row forwards wherever the exact value is neither 0 nor a rounding tie.  The LayerNorm backward divides by C: its dX is
held within 1/2 ulp_bf16(exact) + ((1 + 2^-24)^n - 1) A (fp32 modes: without the bf16 term), A the absolute sum of its terms and
n the number of fp32 roundings on the longest path of a term (exact_ln_reference.n_ln_bwd: 7 one-pass, 8 composed, 9 in the fp32
modes, whose wide shapes are run as two halves; 3 more with the forward kernel's statistics).  Tokens whose dY row is zero come
back exactly 0 / dX_add / dY.
"""
import ctypes

import pytest
import torch

import exact_ln_reference as L
import exact_reference as E
from util import ACT_GELU, GuardedWorkspace, Wide, ln_stats

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16, "f32x3": torch.float32}
PAD, FILL = 8, 3.0
TC = ("token", "channel")


def _scope(mode):
    from rdst_amd import ops
    return ops.compute_scope({"f32": ops.F32, "f32x3": ops.F32X3, "bf16": None}[mode])


def _code(mode):
    from rdst_amd import _lib
    return {"f32": _lib.F32, "bf16": _lib.BF16, "f32x3": _lib.F32X3}[mode]


def _dev(t, dtype, grad=False, wide=False):
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


def _dx_tol(exact, A, n, dt, rows=None, g=None, rstd=None):
    """1/2 ulp_bf16 + ((1 + 2^-24)^n - 1) A; bf16 behind a LayerNorm: a kernel that keeps x-hat in fp32 has x-hat = sigma (1 - e) in
    x-hat mean(g x-hat), twice (L.unnarrowed)."""
    tol = L.roundings(n) * A
    if dt != torch.bfloat16:
        return tol
    if rows is not None:
        s2 = (g.double() * rows["sigma"]).mean(1, keepdim=True).abs()
        tol = tol + rstd.double().reshape(-1, 1) * 2 * L.unnarrowed(rows)[:, None] * s2
    return tol + E.bf16_half_ulp(exact)


def _check_ln_grads(got, ref, op, gy, name, asserted, mode, sc, onepass, tag):
    """dW, dbias, d(gamma), d(beta): exact - but for dW and d(gamma) of the COMPOSED bf16 backward (L.ln_onepass false) on the draw
    that has rows of s < 8 (L.ln_wgrad_tol)."""
    soft = L.ln_wgrad_tol(op, gy, sc) if (mode == "bf16" and name == "thin" and not onepass) else {}
    for k in asserted:
        if k in ("y", "dx"):
            continue
        names = ("out", "in") if k == "dw" else ("channel",)
        if k in soft:
            E.assert_within(got[k], ref[k], soft[k], names, f"{tag}: {k}")
        else:
            E.assert_equal(got[k], E.expect(ref[k], torch.float32), names, f"{tag}: {k}")


def _check_y(got, hard, slack, names, tag):
    """bf16 y of a forward that works on raw rows: equal to bf16(hard) except where the hard value is 0 or not a bf16 number (a
    tie candidate), and within 1/2 ulp + slack everywhere."""
    want = E.expect(hard, torch.bfloat16)
    bad = got.detach().cpu() != want
    loose = (hard == 0) | (hard.float().bfloat16().double() != hard)
    assert not bool((bad & ~loose).any()), f"{tag}: " + "; ".join(E.first_mismatches(torch.where(loose, want, got.detach().cpu()), want, names))
    E.assert_within(got, hard, E.bf16_half_ulp(hard) + slack, names, tag)


def _idle(M, rows):
    idle = torch.ones(M, dtype=torch.bool)
    idle[rows] = False
    return idle


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


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm + Linear through ops.ln_linear
# ---------------------------------------------------------------------------------------------------------------------
def run_ln_linear(op, gy, mode, wide, sc):
    from rdst_amd import ops
    dt = DTYPE[mode]
    xg, xbuf = _dev(op["rows"]["x"], dt, True, wide)
    rg, rbuf = _dev(op["res"], dt, False, wide)
    P = {k: _dev(op[k], torch.float32, True)[0] for k in ("gamma", "beta", "w", "b")}
    with _scope(mode):
        y = ops.ln_linear(xg, P["gamma"], P["beta"], P["w"], P["b"], residual=rg, out_scale=sc)
    y.backward(gy.to(DEV).to(dt))
    torch.cuda.synchronize()
    ok = _untouched(xbuf, op["rows"]["x"], dt) and _untouched(rbuf, op["res"], dt)
    return {"y": y.detach(), "dx": xg.grad, "dw": P["w"].grad, "db": P["b"].grad, "dlw": P["gamma"].grad, "dlb": P["beta"].grad}, ok


@pytest.mark.parametrize("sc", L.SCALES)
@pytest.mark.parametrize("mode", L.MODES)
@pytest.mark.parametrize("M,K,N", L.LN_LINEAR_SHAPES)
def test_ln_linear_exact(M, K, N, mode, sc):
    """fp32, fp32x3: y, dW, dbias, d(gamma), d(beta) exact.  bf16: y equal to bf16(exact) but for exact zeros and ties
    (_check_y); where the one-pass backward runs (L.ln_onepass: out_scale 1 and M K >= N (K + 1)) dW, dbias, d(gamma), d(beta)
    exact on the thinned draw, the s = 1, 2 rows included; in the composed backward (x-hat in fp32) exact over rows of s >= 8 and
    within L.ln_wgrad_tol with s = 1, 2.
    dX within the bound, n = L.n_ln_bwd + 3 (the statistics are the forward kernel's)."""
    dt = DTYPE[mode]
    op = L.ln_linear_case(M, K, N, mode)
    rows = op["rows"]
    rstd = L.true_rstd(rows["s"]) if mode == "bf16" else 1.0 / rows["s"]
    one = L.ln_onepass(mode, sc, M, K, N)
    n = L.n_ln_bwd(mode, sc, M, K, N) + L.N_FWD_STATS
    for name, gy, trows in op["draws"]:
        asserted = L.ln_linear_asserted(mode, name)
        L.check_ln_rules(op, gy, asserted, mode, sc)
        ref = L.ln_linear_hard(rows, op["gamma"], op["beta"], op["w"], op["b"], op["res"], gy, sc)
        dx, A = L.ln_dx(ref["g"], rows["sigma"], rstd)
        if mode != "bf16":
            A = L.ln_dx_abs_halves(op, gy, sc, rstd)
        tol = _dx_tol(dx, A, n, dt) if one else _dx_tol(dx, A, n, dt, rows, ref["g"], rstd)
        for wide in (False, True):
            tag = f"ln_linear {mode} ({M},{K},{N}) s={sc} dY={name} {'wide' if wide else 'compact'}"
            got, ok = run_ln_linear(op, gy, mode, wide, sc)
            assert ok, f"{tag}: an input buffer was written"
            if mode == "bf16":
                _check_y(got["y"], ref["y"], L.ln_y_tol(op, sc), TC, f"{tag}: y")
            else:
                E.assert_equal(got["y"], E.expect(ref["y"], dt), TC, f"{tag}: y")
            E.assert_within(got["dx"], dx, tol, TC, f"{tag}: dX")
            _check_ln_grads(got, ref, op, gy, name, asserted, mode, sc, one, tag)
            if trows is not None:
                assert bool((got["dx"].cpu()[_idle(M, trows)] == 0).all()), f"{tag}: dX is nonzero where dY is zero"


# ---------------------------------------------------------------------------------------------------------------------
# ... and its backward through the C entry point: statistics handed in, dX_add, column slices, the guarded workspace
# ---------------------------------------------------------------------------------------------------------------------
def entry_stats(rows):
    """What the test hands to rdst_ln_linear_bwd: the float32 emulation of what the forward kernels form (L.emulate_stats, the
    contracted formula): (m, 1 / s) exactly at s >= 8, so that x-hat = (x - m) / s is +-1 in fp32 too - the composed backward keeps
    x-hat in fp32 registers even in bf16; a float64 rstd, one ulp below 1 / s, already shows there as 2^-24 in dW."""
    mean, rstd = L.emulate_stats(rows["x"], "fma")
    return torch.stack([mean, rstd], 1).contiguous()


def run_ln_linear_bwd_entry(op, gy, stats, mode, wide, sc):
    from rdst_amd import _lib
    lib = _lib.load()
    dt = DTYPE[mode]
    M, K = op["rows"]["x"].shape
    N = op["w"].shape[0]
    P = {k: op[k].to(DEV).contiguous() for k in ("gamma", "beta", "w")}
    sg = stats.to(DEV).contiguous()
    xo, gyo, addo = _Slot(op["rows"]["x"], dt, "x", wide), _Slot(gy, dt, "dy", wide), _Slot(op["add"], dt, "add", wide)
    dxo = _Slot(torch.full((M, K), float("nan")), dt, "dx", wide)
    out = {"dw": torch.full((N, K), float("nan"), device=DEV), "db": torch.full((N,), float("nan"), device=DEV),
           "dlw": torch.full((K,), float("nan"), device=DEV), "dlb": torch.full((K,), float("nan"), device=DEV)}
    nb = lib.rdst_ln_linear_bwd_workspace(M, K, N)
    wsp = GuardedWorkspace(nb, DEV)
    rc = lib.rdst_ln_linear_bwd(xo.ptr, xo.ld, P["gamma"].data_ptr(), P["beta"].data_ptr(), sg.data_ptr(), 0, P["w"].data_ptr(), gyo.ptr,
                                gyo.ld, dxo.ptr, dxo.ld, addo.ptr, addo.ld, out["dw"].data_ptr(), out["db"].data_ptr(),
                                out["dlw"].data_ptr(), out["dlb"].data_ptr(), wsp.ptr(), nb, M, K, N, sc, _code(mode),
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, f"rdst_ln_linear_bwd refused, rc={rc} {lib.rdst_last_error().decode(errors='replace')}"
    out["dx"] = dxo.t
    return out, wsp.intact(), dxo.intact(), xo.intact() and gyo.intact() and addo.intact()


@pytest.mark.parametrize("sc", L.SCALES)
@pytest.mark.parametrize("mode", L.MODES)
@pytest.mark.parametrize("M,K,N", L.LN_LINEAR_SHAPES)
def test_ln_linear_bwd_entry_exact(M, K, N, mode, sc):
    """dW, dbias, d(gamma), d(beta) exact (bf16: as in test_ln_linear_exact); dX = dX_add + ... within the bound with
    n = L.n_ln_bwd (7 in the one-pass kernels, 8 in the composed backward); idle tokens exactly dX_add."""
    from rdst_amd import _lib
    lib = _lib.load()
    dt = DTYPE[mode]
    op = L.ln_linear_case(M, K, N, mode)
    rows = op["rows"]
    stats = entry_stats(rows)
    one = L.ln_onepass(mode, sc, M, K, N)
    n = L.n_ln_bwd(mode, sc, M, K, N)
    prev = lib.rdst_side_enable(0)
    try:
        for name, gy, trows in op["draws"]:
            asserted = [k for k in L.ln_linear_asserted(mode, name) if k != "y"]
            L.check_ln_rules(op, gy, asserted, mode, sc)
            ref = L.ln_linear_hard(rows, op["gamma"], op["beta"], op["w"], op["b"], None, gy, sc)
            dx, A = L.ln_dx(ref["g"], rows["sigma"], stats[:, 1], op["add"])
            if mode != "bf16":
                A = L.ln_dx_abs_halves(op, gy, sc, stats[:, 1], op["add"])
            tol = _dx_tol(dx, A, n, dt) if one else _dx_tol(dx, A, n, dt, rows, ref["g"], stats[:, 1])
            for wide in (False, True):
                tag = f"rdst_ln_linear_bwd {mode} ({M},{K},{N}) s={sc} dY={name} {'wide' if wide else 'compact'}"
                got, ws_ok, dx_ok, in_ok = run_ln_linear_bwd_entry(op, gy, stats, mode, wide, sc)
                assert ws_ok, f"{tag}: a workspace sentinel was overwritten"
                assert dx_ok, f"{tag}: columns outside the dX slice were overwritten"
                assert in_ok, f"{tag}: an input buffer was written"
                E.assert_within(got["dx"], dx, tol, TC, f"{tag}: dX")
                _check_ln_grads(got, ref, op, gy, name, asserted, mode, sc, one, tag)
                if trows is not None:
                    idle = _idle(M, trows)
                    assert torch.equal(got["dx"].cpu()[idle], op["add"][idle].to(dt)), f"{tag}: dX differs from dX_add where dY is zero"
    finally:
        lib.rdst_side_enable(prev)


# ---------------------------------------------------------------------------------------------------------------------
# GELU + Linear + residual (fc2 of the composed Mlp) through ops.ln_linear: everything exact
# ---------------------------------------------------------------------------------------------------------------------
def run_gelu_linear(op, gy, mode, wide, sc):
    from rdst_amd import ops
    dt = DTYPE[mode]
    xg, xbuf = _dev(op["h"], dt, True, wide)
    rg, rbuf = _dev(op["res"], dt, False, wide)
    wg, _ = _dev(op["w"], torch.float32, True)
    bg, _ = _dev(op["b"], torch.float32, True)
    with _scope(mode):
        y = ops.ln_linear(xg, None, None, wg, bg, in_act=ACT_GELU, residual=rg, out_scale=sc)
    y.backward(gy.to(DEV).to(dt))
    torch.cuda.synchronize()
    ok = _untouched(xbuf, op["h"], dt) and _untouched(rbuf, op["res"], dt)
    return {"y": y.detach(), "dx": xg.grad, "dw": wg.grad, "db": bg.grad}, ok


@pytest.mark.parametrize("sc", L.SCALES)
@pytest.mark.parametrize("mode", L.MODES)
@pytest.mark.parametrize("M,K,N", L.GELU_LINEAR_SHAPES)
def test_gelu_linear_exact(M, K, N, mode, sc):
    """gelu_erf / gelu_erf_grad (fp32) and gelu_fast / gelu_grad_fast (bf16, fp32x3) at h = 0 and |h| >= 16: y, dX, dW, dbias exact."""
    dt = DTYPE[mode]
    op = L.gelu_linear_case(M, K, N, mode)
    for name, gy, trows in op["draws"]:
        asserted = L.gelu_linear_asserted(mode, name)
        L.check_gelu_rules(op, gy, asserted, mode, sc)
        ref = L.gelu_linear_hard(op["h"], op["w"], op["b"], op["res"], gy, None, sc)
        for wide in (False, True):
            tag = f"GELU Linear {mode} ({M},{K},{N}) s={sc} dY={name} {'wide' if wide else 'compact'}"
            got, ok = run_gelu_linear(op, gy, mode, wide, sc)
            assert ok, f"{tag}: an input buffer was written"
            for k in asserted:
                want = E.expect(ref[k], dt if k in ("y", "dx") else torch.float32)
                E.assert_equal(got[k], want, ("out", "in") if k == "dw" else TC if k != "db" else ("channel",), f"{tag}: {k}")
            if trows is not None:
                assert bool((got["dx"].cpu()[_idle(M, trows)] == 0).all()), f"{tag}: dX is nonzero where dY is zero"


# ---------------------------------------------------------------------------------------------------------------------
# the fused Mlp forward, rdst_mlp_fwd, on its three routes
# ---------------------------------------------------------------------------------------------------------------------
MLP_ROUTES = ("pack", "null", "prepacked")


def run_mlp_fwd(op, route, wide):
    from rdst_amd import _lib
    lib = _lib.load()
    M, C = op["rows"]["x"].shape
    hid = op["w1"].shape[0]
    P = {k: op[k].to(DEV).contiguous() for k in ("gamma", "beta", "w1", "b1", "w2", "b2")}
    xo = _Slot(op["rows"]["x"], torch.bfloat16, "x", wide)
    yo = _Slot(torch.full((M, C), float("nan")), torch.bfloat16, "dx", wide)
    stats = torch.full((M, 2), float("nan"), dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    nws = lib.rdst_mlp_fwd_workspace(C, hid)
    wsp, wptr, wbytes = None, None, 0
    if route != "null":
        wsp = GuardedWorkspace(nws, DEV)
        wptr, wbytes = wsp.ptr(), nws
    if route == "prepacked":
        jobs = (_lib.PackJob * 2)()
        jobs[0].kind, jobs[0].W, jobs[0].gamma, jobs[0].beta, jobs[0].bias = (_lib.CONSTANTS["PACK_LINEAR"], P["w1"].data_ptr(),
                                                                              P["gamma"].data_ptr(), P["beta"].data_ptr(), P["b1"].data_ptr())
        jobs[0].out, jobs[0].N, jobs[0].K, jobs[0].s = wptr, hid, C, 1.0
        jobs[1].kind, jobs[1].W, jobs[1].gamma, jobs[1].beta, jobs[1].bias = (_lib.CONSTANTS["PACK_LINEAR"], P["w2"].data_ptr(), None, None,
                                                                              P["b2"].data_ptr())
        jobs[1].out, jobs[1].N, jobs[1].K, jobs[1].s = wptr + lib.rdst_ln_linear_fwd_workspace(C, hid), C, hid, 1.0
        _lib.check(lib.rdst_pack_batch(ctypes.cast(jobs, ctypes.c_void_p), 2, st), "rdst_pack_batch")
        wbytes = _lib.PREPACKED
    _lib.check(lib.rdst_mlp_fwd(xo.ptr, xo.ld, P["gamma"].data_ptr(), P["beta"].data_ptr(), P["w1"].data_ptr(), P["b1"].data_ptr(),
                                P["w2"].data_ptr(), P["b2"].data_ptr(), yo.ptr, yo.ld, stats.data_ptr(), wptr, wbytes, M, C, hid, _lib.BF16, st),
               "rdst_mlp_fwd")
    torch.cuda.synchronize()
    ok = xo.intact() and yo.intact() and (wsp is None or wsp.intact()) and torch.equal(xo.t.cpu(), op["rows"]["x"].bfloat16())
    return yo.t, stats, ok


def mlp_fwd_routes(C, hid):
    from rdst_amd import _lib
    return MLP_ROUTES if _lib.load().rdst_mlp_fwd_packable(C, hid, _lib.BF16) else ("null",)


@pytest.mark.parametrize("M,C,hid", L.MLP_FWD_SHAPES)
def test_mlp_fwd_exact(M, C, hid):
    """Every route: y equal to bf16(hard y) but for exact zeros and ties, and within 1/2 ulp + L.mlp_y_tol there (the forwards
    work on raw rows); stats[:, 0] = m exactly; stats[:, 1] within L.rstd_tol of the float64 rstd (4 ulps behind 1 / sqrtf, 6
    behind the reciprocal square root) and, on the route without a workspace where every 16-byte chunk of a row has a power-of-two
    length (C = 60, 90, 120, 124: the chunk sums are exact), EQUAL to the float32 emulation of mlp_mfma.hip:781-793."""
    op = L.mlp_case(M, C, hid)
    rows = op["rows"]
    L.check_mlp_rules(op, op["dy"], ())
    ref = op["hard_dense"]
    slack = L.mlp_y_tol(op, ref)
    rstd = L.true_rstd(rows["s"])
    for route in mlp_fwd_routes(C, hid):
        for wide in (False, True):
            tag = f"rdst_mlp_fwd ({M},{C},{hid}) route={route} {'wide' if wide else 'compact'}"
            y, stats, ok = run_mlp_fwd(op, route, wide)
            assert ok, f"{tag}: x, a column outside the slices or a workspace sentinel was written"
            _check_y(y, ref["y"], slack, TC, f"{tag}: y")
            E.assert_equal(stats[:, 0], rows["m"].float(), ("token",), f"{tag}: mean")
            E.assert_within(stats[:, 1], rstd, L.rstd_tol(rows, C, route), ("token",), f"{tag}: rstd")
            if route == "null" and L.chunks_exact(C):
                E.assert_equal(stats[:, 1], L.emulate_stats(rows["x"], "fma")[1], ("token",), f"{tag}: rstd against its float32 emulation")


# ---------------------------------------------------------------------------------------------------------------------
# the fused Mlp backward, rdst_mlp_bwd
# ---------------------------------------------------------------------------------------------------------------------
MLP_GRADS = ("dw1", "db1", "dw2", "db2", "dlw", "dlb")


def run_mlp_bwd(op, gy, stats, wide):
    from rdst_amd import _lib
    lib = _lib.load()
    M, C = op["rows"]["x"].shape
    hid = op["w1"].shape[0]
    P = {k: op[k].to(DEV).contiguous() for k in ("gamma", "beta", "w1", "b1", "w2")}
    sg = stats.to(DEV).contiguous()
    xo, gyo = _Slot(op["rows"]["x"], torch.bfloat16, "x", wide), _Slot(gy, torch.bfloat16, "dy", wide)
    dxo = _Slot(torch.full((M, C), float("nan")), torch.bfloat16, "dx", wide)
    shape = {"dw1": (hid, C), "db1": (hid,), "dw2": (C, hid), "db2": (C,), "dlw": (C,), "dlb": (C,)}
    out = {k: torch.full(shape[k], float("nan"), device=DEV) for k in MLP_GRADS}
    nb = lib.rdst_mlp_bwd_workspace(M, C, hid)
    wsp = GuardedWorkspace(nb, DEV)
    _lib.check(lib.rdst_mlp_bwd(xo.ptr, xo.ld, P["gamma"].data_ptr(), P["beta"].data_ptr(), sg.data_ptr(), P["w1"].data_ptr(),
                                P["b1"].data_ptr(), P["w2"].data_ptr(), gyo.ptr, gyo.ld, dxo.ptr, dxo.ld, *(out[k].data_ptr() for k in MLP_GRADS),
                                wsp.ptr(), nb, M, C, hid, _lib.BF16, torch.cuda.current_stream().cuda_stream), "rdst_mlp_bwd")
    torch.cuda.synchronize()
    out["dx"] = dxo.t
    return out, wsp.intact(), dxo.intact(), xo.intact() and gyo.intact()


@pytest.mark.parametrize("M,C,hid", L.MLP_BWD_SHAPES)
def test_mlp_bwd_exact(M, C, hid):
    """Thinned dY (R3: the slabs are bf16): dW1, db1, dW2, db2, d(gamma), d(beta) exact, idle tokens exactly dY; dX within the
    bound with n = 8 on the thinned and on the dense draw (statistics from float64)."""
    from rdst_amd import _lib
    lib = _lib.load()
    assert lib.rdst_mlp_fused_supported(C, hid, _lib.BF16) == 1
    op = L.mlp_case(M, C, hid)
    rows = op["rows"]
    stats = ln_stats(rows["x"])
    prev = lib.rdst_side_enable(0)
    try:
        for name, gy, ref in (("dense", op["dy"], op["hard_dense"]), ("thin", op["thin"], op["hard_thin"])):
            asserted = MLP_GRADS if name == "thin" else ()
            L.check_mlp_rules(op, gy, asserted)
            dx, A = L.ln_dx(ref["g"], rows["sigma"], stats[:, 1], gy)
            for wide in (False, True):
                tag = f"rdst_mlp_bwd ({M},{C},{hid}) dY={name} {'wide' if wide else 'compact'}"
                got, ws_ok, dx_ok, in_ok = run_mlp_bwd(op, gy, stats, wide)
                assert ws_ok, f"{tag}: a workspace sentinel was overwritten"
                assert dx_ok, f"{tag}: columns outside the dX slice were overwritten"
                assert in_ok, f"{tag}: an input buffer was written"
                E.assert_within(got["dx"], dx, _dx_tol(dx, A, L.N_LN_BWD, torch.bfloat16), TC, f"{tag}: dX")
                for k in asserted:
                    E.assert_equal(got[k], E.expect(ref[k], torch.float32), ("out", "in") if k in ("dw1", "dw2") else ("channel",), f"{tag}: {k}")
                if name == "thin":
                    idle = _idle(M, op["thin_rows"])
                    assert torch.equal(got["dx"].cpu()[idle], gy[idle].bfloat16()), f"{tag}: dX differs from dY where dY is zero"
    finally:
        lib.rdst_side_enable(prev)
