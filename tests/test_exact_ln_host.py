"""The references and guards of test_exact_ln_gpu.py, on the CPU: the hard LayerNorm rows keep their promises (exact mean and
rstd under a float32 emulation of every formula the kernels use, the contracted one included), every case and draw the GPU
module uses satisfies R1 - R3 and its class shares, the hard evaluation equals the float64 definition (eps = 0: to 1e-9 of a
quantum; eps = 1e-5: within the leak eps allows), and five mutations of the fused-Mlp results show what the exact comparison
catches.  The gated tests of test_mlp_gpu.py DO see most of these slips at their own sizes (1189 .. 4096 tokens); a relative-L2
gate loses them as the token count grows, which test_mutations_mlp shows at 65573 tokens, a size no gated test runs."""
import numpy as np
import pytest
import torch

import exact_ln_reference as L
import exact_reference as E
from oracle import rdst_oracle as O
from util import rand

MLP_GRADS = ("dw1", "db1", "dw2", "db2", "dlw", "dlb")


# ---------------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", L.MODES)
@pytest.mark.parametrize("C", (60, 62, 90, 120, 124))
def test_ln_rows_keep_their_promises(C, mode):
    M = 133
    rows = L.ln_rows(M, C, mode, 11)
    x, m, s, sigma = rows["x"].double(), rows["m"], rows["s"], rows["sigma"]
    assert torch.equal(x, m[:, None] + s[:, None] * sigma) and bool((sigma.abs() == 1).all()) and bool((sigma.sum(1) == 0).all())
    assert torch.equal(x.sum(1), C * m) and torch.equal(((x - m[:, None]) ** 2).sum(1), C * s * s)        # exact integer sums
    assert s[2] == 64 and s[3] == (1 if mode == "bf16" else L.exact_scales(C, mode)[0])
    assert mode != "bf16" or E.is_bf16(rows["x"])
    assert bool((m != 0).any()) and m.abs().max() > 16, "the means are not limited to 0"
    for a, b in rows["pairs"]:          # same pattern and scale, another mean: rows 0 / 1 and the rows around every tile border
        assert torch.equal(sigma[a], sigma[b]) and s[a] == s[b] and m[a] != m[b]
    assert (0, 1) in rows["pairs"] and (31, 32) in rows["pairs"] and (127, 128) in rows["pairs"]
    for route in L.STAT_ROUTES:         # the float32 emulation of each formula gives (m, 1 / s)
        mean, rstd = L.emulate_stats(rows["x"], route)
        assert torch.equal(mean.double(), m)
        big = s >= 8
        assert torch.equal(rstd.double()[big], 1.0 / s[big])
        # bf16 only: at s < 8 rstd is not 1 / s, and x-hat narrowed to bf16 is exactly +-1 all the same
        xh = ((rows["x"] - mean[:, None]) * rstd[:, None]).bfloat16().double()
        assert mode != "bf16" or torch.equal(xh, sigma)
        assert mode == "bf16" or bool(big.all())
    r2 = L.ln_rows(M, C, mode, 11)
    assert torch.equal(r2["x"], rows["x"]) and not torch.equal(L.ln_rows(M, C, mode, 12)["x"], rows["x"])


def test_exact_means_and_scales():
    """The means and scales whose statistics are exact in float32 on every formula, the contracted var * invK + eps included."""
    for K in (62, 90, 124, 180):
        assert len(L.exact_means(K)) == 513                       # every |m| <= 256
    want = set([0, 1, 2, 4, 8, 9, 256] + list(range(16, 19)) + list(range(32, 37)) + list(range(64, 74)) + list(range(128, 147)))
    for K in (60, 120, 240):
        assert set(np.abs(L.exact_means(K)).tolist()) == want
    for K in (60, 90, 120):
        assert L.exact_scales(K, "f32") == [16, 32, 64, 128] and L.exact_scales(K, "bf16") == [1, 2, 16, 32, 64, 128]
        sq, inv = np.array([K * 64.0], dtype=np.float32), np.float32(1.0) / np.float32(K)
        assert L._rstd32(sq * inv)[0] == np.float32(0.125) and L._rstd32(fused=(sq, inv))[0] != np.float32(0.125)   # s = 8: uncontracted yes, contracted no
    for K in (62, 124):
        assert L.exact_scales(K, "f32") == [8, 16, 32, 64, 128]


def test_hard_gelu_points():
    """GELU and GELU' at the hard points in float64, and in float32 with the formulas of common.h (erff / expf as the host has
    them): 0 and 1/2 at h = 0; max(h, 0) and 0 / 1 at |h| >= 16; and why a quantum of 8 is not enough."""
    h = torch.tensor([0.0, 16.0, -16.0, 48.0, -4080.0, 4080.0], dtype=torch.float64)
    a, d = L.hard_gelu(h)
    hr = h.clone().requires_grad_(True)
    O.gelu(hr).sum().backward()
    assert (O.gelu(h) - a).abs().max().item() < 1e-50 and (hr.grad - d).abs().max().item() < 1e-50
    h32 = h.float()
    erf = torch.erf(h32 * np.float32(0.70710678118654752440))
    assert torch.equal(0.5 * h32 * (1 + erf), a.float())                                                  # gelu_erf
    g32 = 0.5 * (1 + erf) + h32 * np.float32(0.39894228040143267794) * torch.exp(-0.5 * h32 * h32)
    assert torch.equal(g32, d.float())                                                                    # gelu_erf_grad
    m8 = torch.tensor([-8.0])
    g8 = 0.5 * (1 + torch.erf(m8 * np.float32(0.70710678118654752440))) + m8 * np.float32(0.39894228040143267794) * torch.exp(-0.5 * m8 * m8)
    assert g8.item() != 0.0 and abs(g8.item()) < 1e-12
    # the fp16 table of gelu_tab_fill: entry 256 is (1/2, slope, 1/2, slope) and the clamped ends are (0, 0) / (1, 0)
    u = torch.tensor([-8.0, 0.0, 8.0 - 1 / 32], dtype=torch.float64)
    phi = (0.5 * torch.erfc(-u * 0.70710678118654752440)).half()
    assert phi.tolist() == [0.0, 0.5, 1.0]
    for cls in ((L.hard_h((64, 33), 5) == 0), (L.hard_h((64, 33), 5) >= 16), (L.hard_h((64, 33), 5) <= -16)):
        assert cls.double().mean().item() > 0.2


# ---------------------------------------------------------------------------------------------------------------------
# every case of the GPU module: preconditions, hard against the definition
# ---------------------------------------------------------------------------------------------------------------------
def _close(true, hard, quantum, what):
    """1e-9 of a quantum, plus what float64 autograd itself rounds on sums of this size (1e-12 of the largest element)."""
    worst = (true - hard).abs().max().item()
    assert worst < 1e-9 * quantum + 1e-12 * hard.abs().max().item(), f"{what}: hard and float64 differ by {worst:.3e}"


@pytest.mark.parametrize("sc", L.SCALES)
@pytest.mark.parametrize("mode", L.MODES)
@pytest.mark.parametrize("M,K,N", L.LN_LINEAR_SHAPES)
def test_ln_linear_cases(M, K, N, mode, sc):
    op = L.ln_linear_case(M, K, N, mode)
    rows = op["rows"]
    q = E.LO_Q if op["config"] == "w_hilo" else 1.0
    for name, gy, trows in op["draws"]:
        asserted = L.ln_linear_asserted(mode, name)
        L.check_ln_rules(op, gy, asserted, mode, sc)
        hard = L.ln_linear_hard(rows, op["gamma"], op["beta"], op["w"], op["b"], op["res"], gy, sc)
        for k in ("y", "dw", "db", "dlw", "dlb"):
            E.expect(hard[k], torch.float32)                     # an fp32 number (asserted inside)
        true0 = L.ln_linear_true(rows["x"], op["gamma"], op["beta"], op["w"], op["b"], op["res"], gy, sc, op["add"], eps=0.0)
        for k in ("y", "dw", "db", "dlw", "dlb"):
            _close(true0[k], hard[k], 0.5 * sc * q, f"{mode} ({M},{K},{N}) {name}: {k}")
        dx, A = L.ln_dx(hard["g"], rows["sigma"], 1.0 / rows["s"], op["add"])
        assert ((true0["dx"] - dx).abs() <= 1e-12 * A + 1e-300).all()
        # with eps: every output within the leak of its absolute sum; dX against the true rstd, hard x-hat
        true = L.ln_linear_true(rows["x"], op["gamma"], op["beta"], op["w"], op["b"], op["res"], gy, sc, op["add"])
        ab = L.ln_linear_abs(rows, op["gamma"], op["beta"], op["w"], op["b"], op["res"], gy)
        lk = L.leak(rows["s"].min().item())
        for k in ("y", "dw", "dlw"):
            assert (true[k] - hard[k]).abs().max().item() <= lk * ab[k], f"{mode} ({M},{K},{N}) {name}: the leak of eps in {k}"
        dxt, At = L.ln_dx(hard["g"], rows["sigma"], L.true_rstd(rows["s"]), op["add"])
        assert ((true["dx"] - dxt).abs() <= lk * At + 1e-300).all()
        if trows is not None:
            t = trows.tolist()
            assert 0 in t and M - 1 in t and (mode != "bf16" or len(t) <= 256)


@pytest.mark.parametrize("sc", L.SCALES)
@pytest.mark.parametrize("mode", L.MODES)
@pytest.mark.parametrize("M,K,N", L.GELU_LINEAR_SHAPES)
def test_gelu_linear_cases(M, K, N, mode, sc):
    op = L.gelu_linear_case(M, K, N, mode)
    q = E.LO_Q if op["config"] == "w_hilo" else 1.0
    for name, gy, trows in op["draws"]:
        L.check_gelu_rules(op, gy, L.gelu_linear_asserted(mode, name), mode, sc)
        hard = L.gelu_linear_hard(op["h"], op["w"], op["b"], op["res"], gy, op["add"], sc)
        true = L.gelu_linear_true(op["h"], op["w"], op["b"], op["res"], gy, op["add"], sc)
        for k in ("y", "dx", "dw", "db"):
            E.expect(hard[k], torch.float32)
            _close(true[k], hard[k], 0.5 * sc * q, f"{mode} ({M},{K},{N}) {name}: {k}")          # the leak of Phi(-16): nothing


@pytest.mark.parametrize("M,C,hid", sorted(set(L.MLP_FWD_SHAPES + L.MLP_BWD_SHAPES)))
def test_mlp_cases(M, C, hid):
    op = L.mlp_case(M, C, hid)
    rows = op["rows"]
    L.check_mlp_rules(op, op["dy"], ())
    L.check_mlp_rules(op, op["thin"], MLP_GRADS)
    t = op["thin_rows"].tolist()
    assert 0 in t and M - 1 in t                                  # the last token of the ragged tile carries a gradient
    E.expect(op["hard_dense"]["y"], torch.bfloat16)
    for k in MLP_GRADS:
        E.expect(op["hard_thin"][k], torch.float32)
    # int64: h in units of 16 and dW2 in units of 16 from integer matrices
    sig, t1 = rows["sigma"].long(), (op["w1"] * op["gamma"] / 16).double().round().long()
    h16 = sig @ t1.t() + ((op["b1"].double() + op["w1"].double() @ op["beta"].double()) / 16).round().long()
    assert torch.equal(h16.double() * 16, op["hard_dense"]["h"])
    assert torch.equal((op["thin"].long().t() @ h16.clamp_min(0)).double() * 16, op["hard_thin"]["dw2"])
    if M > 20000:
        return
    for gy, hard in ((op["thin"], op["hard_thin"]), (op["dy"], op["hard_dense"])):
        true0 = L.mlp_true(op, gy, eps=0.0)
        for k in ("y",) + MLP_GRADS:
            _close(true0[k], hard[k], 0.5, f"({M},{C},{hid}): {k}")
        dx, A = L.ln_dx(hard["g"], rows["sigma"], 1.0 / rows["s"], gy)
        assert ((true0["dx"] - dx).abs() <= 1e-10 * A + 1e-11).all()


# ---------------------------------------------------------------------------------------------------------------------
# mutations: what the exact comparison catches at any size, and from which size on a relative-L2 gate of 8e-3 stops seeing it
# ---------------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return ((a - b).norm() / b.norm()).item()


def _gate_inputs(M=32 * 37 + 5):
    """The operands of test_mlp_gpu.py (its first case, M = 32 * 37 + 5: a ragged last tile; or the same recipe at another M)."""
    C, hid = 60, 120
    x, gy = rand((M, C), 1).bfloat16().double(), rand((M, C), 2).bfloat16().double()
    lw, lb = (1 + 0.1 * rand((C,), 3)).double(), (0.1 * rand((C,), 4)).double()
    w1, b1 = rand((hid, C), 5, C ** -0.5).double(), (0.1 * rand((hid,), 6)).double()
    w2, b2 = rand((C, hid), 7, hid ** -0.5).double(), (0.1 * rand((C,), 8)).double()
    return x, gy, lw, lb, w1, b1, w2, b2


def _mlp64(x, gy, lw, lb, w1, b1, w2, b2, stats=None, mask=None):
    """Forward and backward of the Mlp half in float64, written out, with hooks for the mutations: `stats` (mean, rstd) per
    row instead of the row's own, `mask` = GELU' per (token, unit) instead of the true one."""
    mean = x.mean(1, keepdim=True) if stats is None else stats[0]
    rstd = (x.var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt() if stats is None else stats[1]
    xh = (x - mean) * rstd
    z = xh * lw + lb
    h = z @ w1.t() + b1
    a = O.gelu(h)
    hr = h.clone().requires_grad_(True)
    O.gelu(hr).sum().backward()
    d = hr.grad if mask is None else mask
    y = x + a @ w2.t() + b2
    u = d * (gy @ w2)
    G = u.t() @ xh
    db1 = u.sum(0)
    dz = u @ w1
    g = dz * lw
    dx = gy + rstd * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    return {"y": y, "dx": dx, "dw1": lw * G + lb * db1[:, None], "db1": db1, "dw2": gy.t() @ a, "db2": gy.sum(0), "dlw": (dz * xh).sum(0),
            "dlb": dz.sum(0), "u": u, "xh": xh, "dz": dz, "G": G, "d": d, "mean": mean, "rstd": rstd}


def test_mutations_mlp():
    """Each slip on the HARD case changes a result that is compared with torch.equal, whatever the number of tokens.  The gates
    of test_mlp_gpu.py (backward: relative L2 <= 8e-3 per output; forward: 1e-2 and 3e-2 max-abs) are evaluated in float64 on that
    module's own operand recipe.  At its 1189 tokens the gated test is NOT blind to these slips: the two one-token slips move
    d(gamma) and db1 by 3e-2 to 4e-2 (asserted below), a dropped beta db^T by 1e-1, a whole tile of it by 1.5e-2.  A slip
    confined to one 32-token tile or one token moves a sum over M tokens by about sqrt(32 / M) or 1 / sqrt(M) of its norm, so
    the same gates evaluated at 65573 tokens - the forward shape of the exact test, a size no gated test runs - pass all
    five; mutation 1 is shown there for one tile's tokens, since the whole term is seen at every size."""
    M, C, hid = 165, 60, 120
    op = L.mlp_case(M, C, hid)
    rows, gt, hard = op["rows"], op["thin"].double(), op["hard_thin"]
    last = M - 1
    assert last in op["thin_rows"].tolist() and M % 32 != 0
    sigma, z = rows["sigma"], op["gamma"].double() * rows["sigma"] + op["beta"].double()
    u, dz = hard["u"], hard["u"] @ op["w1"].double()
    small = _mlp64(*_gate_inputs())
    x, gy, lw, lb, w1, b1, w2, b2 = _gate_inputs(65573)
    ref = _mlp64(x, gy, lw, lb, w1, b1, w2, b2)
    tile = slice(32 * 36, 32 * 37)

    def fires(mut, want, dtype=torch.float32):
        return not torch.equal(E.expect(mut, dtype), E.expect(want, dtype))

    # 1. dW1 without beta db^T: altogether (the gate sees that: beta ~ 0.1 there, 1e-1), and for the tokens of one tile only
    assert fires(op["gamma"].double() * hard["G1"], hard["dw1"])
    tile_h = torch.tensor([t for t in op["thin_rows"].tolist() if t >= 160])
    assert fires(hard["dw1"] - op["beta"].double() * u[tile_h].sum(0)[:, None], hard["dw1"])
    assert _rel(lw * ref["G"], ref["dw1"]) > 8e-3 >= _rel(ref["dw1"] - lb * ref["u"][tile].sum(0)[:, None], ref["dw1"])
    # 2. the last token of the ragged tile left out of d(gamma)
    assert fires(hard["dlw"] - dz[last] * sigma[last], hard["dlw"])
    assert _rel(small["dlw"] - small["dz"][-1] * small["xh"][-1], small["dlw"]) > 8e-3
    assert _rel(ref["dlw"] - ref["dz"][-1] * ref["xh"][-1], ref["dlw"]) <= 8e-3
    # 3. one hidden unit's GELU mask forced to 1 in one 32-token tile
    j = int(((hard["h"][160:] <= -16) & (gt[160:] @ op["w2"].double() != 0)).any(0).nonzero()[0, 0])
    mask = L.hard_gelu(hard["h"])[1].clone()
    mask[160:, j] = 1.0
    um = mask * (gt @ op["w2"].double())
    assert fires(um.sum(0), hard["db1"]) and fires(um.t() @ z, hard["dw1"])
    dmask = ref["d"].clone()
    dmask[tile, 7] = 1.0
    mut = _mlp64(x, gy, lw, lb, w1, b1, w2, b2, mask=dmask)
    for k in ("dx", "dw1", "db1", "dlw", "dlb"):
        assert 0 < _rel(mut[k], ref[k]) <= 8e-3, k
    # 4. one row's (mean, rstd) taken from the next row (rows 0 and 1 of the hard case differ in their mean only)
    a, b = rows["pairs"][0]
    xh_wrong = sigma[a] + (rows["m"][a] - rows["m"][b]) / rows["s"][a]
    h_wrong = (op["gamma"].double() * xh_wrong + op["beta"].double()) @ op["w1"].double().t() + op["b1"].double()
    y_wrong = rows["x"][a].double() + O.gelu(h_wrong) @ op["w2"].double().t() + op["b2"].double()
    assert not torch.equal(y_wrong.float().bfloat16(), op["hard_dense"]["y"][a].float().bfloat16())
    mean, rstd = ref["mean"].clone(), ref["rstd"].clone()
    mean[1000], rstd[1000] = ref["mean"][1001], ref["rstd"][1001]
    mut = _mlp64(x, gy, lw, lb, w1, b1, w2, b2, stats=(mean, rstd))
    assert _rel(mut["y"], ref["y"]) <= 1e-2 and not torch.equal(mut["y"][1000], ref["y"][1000])     # (the max-abs gate of the forward does see this row)
    for k in ("dx", "dw1", "db1", "dw2", "dlw", "dlb"):
        assert 0 < _rel(mut[k], ref[k]) <= 8e-3, k
    # 5. db1 missing one token
    assert fires(hard["db1"] - u[last], hard["db1"]) and bool((u[last] != 0).any())
    assert _rel(small["db1"] - small["u"][-1], small["db1"]) > 8e-3 >= _rel(ref["db1"] - ref["u"][-1], ref["db1"])
