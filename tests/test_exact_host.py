"""The references and guards of the exact-result tests (exact_reference.py, test_exact_gpu.py), on the CPU: the operand
generators keep their promises, every shape and draw the GPU module uses satisfies R1 - R3 and its float64 result equals an
integer computation (int64 on operands scaled to integers; whole tensors where that is cheap, a fixed sample of rows,
pixels and output channels - the first and the last always among them - where it is not), the hard-attention references have
every softmax weight at 0 or a power of two, and four mutations of the references show what the exact comparison catches and
the 2e-2 relative-L2 gate of the other bf16 tests lets through."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_reference as E


# ---------------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------------
def test_generators_keep_their_promises():
    a = E.ints((7, 5), 1, -3, 3)
    assert a.dtype == torch.float32 and a.min() >= -3 and a.max() <= 3 and torch.equal(a, a.round()) and E.is_bf16(a)
    assert torch.equal(a, E.ints((7, 5), 1, -3, 3)) and not torch.equal(a, E.ints((7, 5), 2, -3, 3))      # seeded
    p = E.pos_ints((9, 9), 3, 3)
    assert p.min() >= 1 and p.max() <= 3
    assert torch.equal(F.leaky_relu(p, 0.2), p)
    for positive in (False, True):
        v = E.hilo((64, 33), 4, positive)
        hi, lo = E.split_hilo(v)
        assert bool((hi != 0).all()) and bool((lo != 0).all()) and E.is_bf16(hi) and E.is_bf16(lo) and torch.equal(hi + lo, v)
        assert not E.is_bf16(v)
        assert torch.equal(v / E.LO_Q, (v / E.LO_Q).round()) and (v.abs() / E.LO_Q).max() < 2 ** 16      # 16 significant bits
        assert positive == bool((v > 0).all())
    assert E.is_pow2(0.5) and E.is_pow2(0.25) and E.is_pow2(1.0) and not E.is_pow2(0.7) and not E.is_pow2(0.9)
    assert E.pow2_scale(0.7) == 0.5 and E.pow2_scale(0.9) == 0.25 and E.pow2_scale(1.0) == 1.0


def test_thin_rows():
    x = E.ints((600, 16), 5, -3, 3)
    dy, rows = E.thin_rows(600, 200, 8, 6, E.linear_contrib(x), 256.0)
    rows = rows.tolist()
    for f in (0, 199, 200, 399, 400, 599):          # first and last row of every image, +-1 in every channel
        assert f in rows and bool((dy[f].abs() == 1).all())
    assert set(dy.unique().tolist()) <= {-1.0, 0.0, 1.0}
    idle = torch.ones(600, dtype=torch.bool)
    idle[rows] = False
    assert bool((dy[idle] == 0).all())
    bound = (dy.abs().double().t() @ x.abs().double()).max().item()
    assert bound <= 256 and x[rows].abs().double().sum(0).max().item() <= 256
    assert len(rows) > 100                           # as large as the limit allows: one more row would pass 256 (|x| <= 3)
    assert x[rows].abs().double().sum(0).max().item() > 256 - 3 or len(rows) == 600
    assert len(E.thin_rows(600, 200, 8, 6, E.linear_contrib(x), 1e9)[1]) == 600
    with pytest.raises(AssertionError):              # a limit the forced rows alone break is an error, never a silent drop
        E.thin_rows(600, 200, 8, 6, E.linear_contrib(x), 2.0)


def test_expect_and_mismatch_report():
    e = torch.tensor([[257.0, 258.0], [3.0, -259.0]], dtype=torch.float64)
    assert torch.equal(E.expect(e, torch.float32), e.float())
    assert torch.equal(E.expect(e, torch.bfloat16).float(), torch.tensor([[256.0, 258.0], [3.0, -260.0]]))   # ties to even
    with pytest.raises(AssertionError):
        E.expect(torch.tensor([2.0 ** 24 + 1], dtype=torch.float64), torch.float32)
    got = e.float().clone()
    got[1, 0] = 4.0
    msg = E.first_mismatches(got, e.float(), ("row", "column"))
    assert len(msg) == 1 and "row=1, column=0" in msg[0] and "4.0" in msg[0] and "3.0" in msg[0]
    assert E.first_mismatches(e.float(), e.float(), ("row", "column")) == []
    with pytest.raises(AssertionError, match="row=1, column=0"):
        E.assert_equal(got, e.float(), ("row", "column"), "case")
    h = E.bf16_half_ulp(torch.tensor([0.0, 1.0, 1.5, 2.0, 0.75, -3.0], dtype=torch.float64))
    assert h.tolist() == [0.0, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9, 2.0 ** -7]
    with pytest.raises(AssertionError, match="row=0, column=1"):
        E.assert_within(torch.tensor([[1.0, 2.5]]), torch.tensor([[1.0, 2.0]], dtype=torch.float64), 0.25, ("row", "column"), "case")


# ---------------------------------------------------------------------------------------------------------------------
# the float64 references against integer arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def _i64(t, q):
    s = t.double() / q
    assert torch.equal(s, s.round()), "not a multiple of its quantum"
    return s.long()


def _sample(n, count, seed):
    if n <= count:
        return torch.arange(n)
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(np.unique(np.concatenate([[0, n - 1], g.integers(0, n, count - 2)])))


def _check_linear_int(op, b, res, gy, add, scale, config, ref):
    qx, qw = (E.LO_Q if config == "x_hilo" else 1.0), (E.LO_Q if config == "w_hilo" else 1.0)
    X, Wt, G = _i64(op["x"], qx), _i64(op["w"], qw), _i64(gy, 1.0)
    inv = int(round(1.0 / scale))
    rows, outs = _sample(X.shape[0], 64, 1), _sample(Wt.shape[0], 8, 2)
    y = X[rows] @ Wt.t()                                     # in units of qx qw s
    if b is not None:
        y = y + _i64(b, qx * qw)
    if res is not None:
        y = y + _i64(res[rows], qx * qw) * inv
    assert torch.equal(y.double() * (qx * qw * scale), ref["y"][rows])
    dx = G[rows] @ Wt                                        # in units of qw s
    if add is not None:
        dx = dx + _i64(add[rows], qw) * inv
    assert torch.equal(dx.double() * (qw * scale), ref["dx"][rows])
    assert torch.equal((G[:, outs].t() @ X).double() * (qx * scale), ref["dw"][outs])
    assert torch.equal(G.sum(0).double() * scale, ref["db"])


@pytest.mark.parametrize("M,K,N", E.LINEAR_SHAPES)
def test_linear_cases_are_exact(M, K, N):
    """Both Linear tests of the GPU module (ops.ln_linear: seeds 1000 ..., rdst_ln_linear_bwd: 2000 ...), every mode."""
    for mode in E.MODES:
        for config in E.CONFIGS[mode]:
            hilo_name = {"int": None, "x_hilo": "x", "w_hilo": "w"}[config]
            for vi, (bias, res, scale, act) in enumerate(E.LINEAR_VARIANTS):
                op = E.linear_operands(M, K, N, config, act, 1000 + 10 * vi)
                b, r = (op["b"] if bias else None), (op["res"] if res else None)
                for name, gy, rows, asserted in E.linear_draws(op, N, mode, config, 1000 + 10 * vi):
                    ref = E.linear_ref(op["x"], op["w"], b, r, gy, None, act, scale)
                    E.check_rules({"x": op["x"], "w": op["w"], "b": b, "res": r, "dy": gy}, hilo_name, scale,
                                  E.linear_abs(op["x"], op["w"], b, r, gy, None, config), asserted, mode)
                    _check_linear_int(op, b, r, gy, None, scale, config, ref)
                    for k in asserted:
                        E.expect(ref[k], torch.float32)      # an fp32 number (asserted inside)
            for vi, (act, scale, with_add) in enumerate(E.LINEAR_BWD_VARIANTS):
                op = E.linear_operands(M, K, N, config, act, 2000 + 10 * vi)
                add = op["add"] if with_add else None
                for name, gy, rows, asserted in E.linear_draws(op, N, mode, config, 2000 + 10 * vi):
                    ref = E.linear_ref(op["x"], op["w"], op["b"], None, gy, add, act, scale)
                    E.check_rules({"x": op["x"], "w": op["w"], "dy": gy, "dx_add": add}, hilo_name, scale,
                                  E.linear_abs(op["x"], op["w"], op["b"], None, gy, add, config), [k for k in asserted if k != "y"], mode)
                    _check_linear_int(op, op["b"], None, gy, add, scale, config, ref)
                    if rows is not None and mode == "bf16":
                        assert len(rows) <= 256 and 0 in rows.tolist() and M - 1 in rows.tolist()


def _unshuffle(t, r):
    """(B, H r, W r, c) -> (B, H, W, c r^2) in conv channel order."""
    return t if r == 1 else F.pixel_unshuffle(t.permute(0, 3, 1, 2), r).permute(0, 2, 3, 1)


def _check_conv_int(case, op, rr, gy, config, ref):
    B, H, W, Cin, Cout, k, act, res, scale, r = case
    qx, qw = (E.LO_Q if config == "x_hilo" else 1.0), (E.LO_Q if config == "w_hilo" else 1.0)
    inv = int(round(1.0 / scale))
    X, Wt, G = _i64(op["x"], qx), _i64(op["w"], qw), _i64(_unshuffle(gy, r), 1.0)      # G in the conv geometry (B, H, W, Cout)
    pix = _sample(B * H * W, 256, 3)
    bi, yi, xi = pix // (H * W), (pix // W) % H, pix % W
    y = torch.einsum("nyxi,oiyx->no", E._patches(X, pix, k).long(), Wt) + _i64(op["b"], qx * qw)
    if rr is not None:
        y = y + _i64(_unshuffle(rr, r)[bi, yi, xi], qx * qw) * inv
    assert torch.equal(y.double() * (qx * qw * scale), _unshuffle(ref["y"], r)[bi, yi, xi])
    dx = torch.einsum("nyxo,oiyx->ni", E._patches(G, pix, k).long().flip(1, 2), Wt)       # dX[p] = sum_t dY[p - t + pad] w[t]
    assert torch.equal(dx.double() * (qw * scale), ref["dx"][bi, yi, xi])
    outs = _sample(Cout, 4, 4)
    dw = torch.zeros(len(outs), Cin, k, k, dtype=torch.int64)
    for b in range(B):                                                                     # image by image: the patches of all pixels
        allp = torch.arange(b * H * W, (b + 1) * H * W)
        dw += torch.einsum("no,nyxi->oiyx", G.reshape(-1, Cout)[allp][:, outs], E._patches(X, allp, k).long())
    assert torch.equal(dw.double() * (qx * scale), ref["dw"][outs])
    assert torch.equal(G.reshape(-1, Cout).sum(0).double() * scale, ref["db"])


ALL_CONV = E.CONV_CASES + [(B, H, W, 1, Cout, 3, 0, False, s, 1) for B, H, W, Cout, s in E.HEAD_CONV_CASES]


@pytest.mark.parametrize("case", ALL_CONV, ids=lambda c: "x".join(str(v) for v in c))
def test_conv_cases_are_exact(case):
    B, H, W, Cin, Cout, k, act, res, scale, r = case
    x_grad = case in E.CONV_CASES
    assert E.is_pow2(scale)
    for config in ("int", "x_hilo", "w_hilo"):
        hilo_name = {"int": None, "x_hilo": "x", "w_hilo": "w"}[config]
        qs = E.quanta(config)
        op = E.conv_operands(B, H, W, Cin, Cout, k, act, r, config, 3000)
        rr = op["res"] if res else None
        gy = E.dense_gy(tuple(op["res"].shape), 3005)
        ref = E.conv_ref(op["x"], op["w"], op["b"], rr, gy, act, scale, r)
        bounds = E.conv_abs(op["x"], op["w"], op["b"], rr, gy, r, config)
        _check_conv_int(case, op, rr, gy, config, ref)
        for mode in (m for m in E.MODES if config in E.CONFIGS[m]):
            asserted, dense_w = E.conv_dense_asserted(mode, bounds, x_grad)
            E.check_rules({"x": op["x"], "w": op["w"], "b": op["b"], "res": rr, "dy": gy}, hilo_name, scale, bounds, asserted, mode)
            for k_ in asserted:
                E.expect(ref[k_], torch.float32)
            if dense_w:
                continue
            for s in E.thin_seeds(B, H, W):
                gt, rows = E.conv_thin_gy(op["x"], Cout, k, r, 3100 + s, E.conv_thin_limit(mode, config))
                first = torch.arange(B) * (H * r * W * r)
                assert set(first.tolist()) <= set(rows.tolist()) and set((first + H * r * W * r - 1).tolist()) <= set(rows.tolist())
                tref = E.conv_wgrad_sparse(op["x"], gt, rows, Cout, k, scale, r)
                tb = E.conv_wgrad_sparse(op["x"].abs(), gt.abs(), rows, Cout, k, 1.0, r)
                E.check_rules({"dy": gt}, None, scale, {k_: v.max().item() / qs[k_] for k_, v in tb.items()}, ("dw", "db"), mode)
                if B * H * W < E.LARGE_PIXELS or (s == 0 and mode == "bf16"):   # the written-out sum against autograd on the whole tensor
                    full = E.conv_ref(op["x"], op["w"], op["b"], None, gt, act, scale, r)
                    assert torch.equal(full["dw"], tref["dw"]) and torch.equal(full["db"], tref["db"])
                    if mode == "bf16":
                        _check_conv_int(case, op, None, gt, config, full)


# ---------------------------------------------------------------------------------------------------------------------
# hard attention
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C,heads,ws,shift,kind", E.ATTN_RUNS)
def test_hard_attention_references(B, H, W, C, heads, ws, shift, kind):
    c = E.attn_case(B, H, W, C, heads, ws, shift, kind)
    N = ws * ws
    P = E.attn_weights(c["table"], H, W, heads, ws, shift)
    hard, dev = E.harden(P)
    assert dev <= 1e-30 and c["dev"] == dev                         # every weight 0 or a power of two
    nz = hard[hard > 0]
    assert torch.equal(torch.log2(nz), torch.log2(nz).round()) and torch.equal(hard.sum(-1), torch.ones_like(hard.sum(-1)))
    if kind == "centre":
        assert torch.equal(hard, torch.eye(N, dtype=torch.float64).expand_as(hard))
    if kind == "probe":                                             # one partner (weight 1) or none (1 / N), both occur
        top = hard.amax(-1)
        assert set(top.unique().tolist()) == {1.0, 1.0 / N}
        for h in range(heads):                                      # ... and the partner is the one the table names
            t = int((c["table"][:, h] == 0).nonzero()[0, 0])
            i, j = (hard[0, h] == 1).nonzero().t()
            assert bool((E.O.relative_position_index(ws)[i, j] == t).all())
    vmax = c["qkv"][..., 2 * C:].abs().max().item()
    assert (c["soft_o"] - c["o"]).abs().max().item() <= 1e-38 * vmax           # what the -100 logits leak
    # N O and N dV are integers (scaled-integer form of the reference), and far below 2^24
    for k in ("o", "dv"):
        assert torch.equal(c[k] * N, (c[k] * N).round()) and c["abs_" + k].max().item() * N < 2 ** 24
    assert bool((c["qkv"][..., :C] == 0).all()) and E.is_bf16(c["qkv"]) and E.is_bf16(c["dO"]) and E.is_bf16(c["table"])
    assert c["qkv"][..., C:2 * C].abs().max() > c["qkv"][..., 2 * C:].abs().max()     # k and v told apart by their ranges


# ---------------------------------------------------------------------------------------------------------------------
# mutations: what the exact comparison catches and a 2e-2 relative-L2 gate does not
# ---------------------------------------------------------------------------------------------------------------------
def _gate_silent(mut, ref):
    """The relative-L2 gate of the other bf16 kernel tests (2e-2) on a result rounded to bf16."""
    got = mut.float().bfloat16().double()
    return ((got - ref).norm() / ref.norm()).item() <= 2e-2


def _exact_fires(mut, ref, names):
    a, b = E.expect(mut, torch.bfloat16), E.expect(ref, torch.bfloat16)
    bad = E.first_mismatches(a, b, names)
    return (not torch.equal(a, b)) and len(bad) > 0


def test_mutations_conv():
    """33 x 6 x 256 x 60 -> 60 in bf16 (register-stationary kernels, 16-row strips, a second strip per workgroup)."""
    case = (33, 6, 256, 60, 60, 3, 0, True, 0.5, 1)
    B, H, W, Cin, Cout, k, act, res, scale, r = case
    op = E.conv_operands(B, H, W, Cin, Cout, k, act, r, "int", 3000)
    gy = E.dense_gy(tuple(op["res"].shape), 3005)
    ref = E.conv_ref(op["x"], op["w"], op["b"], op["res"], gy, act, scale, r)
    x, w = op["x"].double(), op["w"].double()
    names = ("image", "row", "column", "channel")
    # 1. one tap dropped at one corner pixel: the centre tap of the last pixel of image 7
    m1 = ref["y"].clone()
    m1[7, H - 1, W - 1] -= scale * (w[:, :, 1, 1] @ x[7, H - 1, W - 1])
    # 2. two channels of one 8-channel chunk swapped in one row
    m2 = ref["y"].clone()
    m2[12, 3, :, [17, 18]] = ref["y"][12, 3, :, [18, 17]]
    # 3. the first row of a strip shifted by one pixel, in one 32-pixel slab and one 8-channel chunk (256 elements; the whole
    #    row, 15360 elements, is a tenth of a percent of the tensor's energy and a 2e-2 gate does see that)
    m3 = ref["y"].clone()
    m3[20, 0, 64:96, 8:16] = ref["y"][20, 0, 63:95, 8:16]
    for i, m in enumerate((m1, m2, m3)):
        assert _exact_fires(m, ref["y"], names), f"mutation {i + 1}: the exact comparison did not fire"
        assert _gate_silent(m, ref["y"]), f"mutation {i + 1}: the relative-L2 gate fired"
    # 4. one pixel lost from dW: on the dense draw (what the 2e-2 gate sees) and on the thinned draw (what bf16 asserts)
    p = 5 * H * W + 2 * W + 77
    lost = scale * torch.einsum("c,yxi->ciyx", gy.reshape(-1, Cout)[p].double(), E._patches(op["x"], torch.tensor([p]), k)[0])
    m4 = ref["dw"] - lost
    assert not torch.equal(m4.float(), ref["dw"].float())
    assert E.first_mismatches(m4.float(), ref["dw"].float(), ("out", "in", "ky", "kx"))
    assert _gate_silent(m4, ref["dw"])
    gt, rows = E.conv_thin_gy(op["x"], Cout, k, r, 3100, E.LIMIT_BF16)
    tref = E.conv_wgrad_sparse(op["x"], gt, rows, Cout, k, scale, r)
    keep = rows[rows != rows[len(rows) // 2]]
    tmut = E.conv_wgrad_sparse(op["x"], gt, keep, Cout, k, scale, r)
    assert not torch.equal(E.expect(tmut["dw"], torch.float32), E.expect(tref["dw"], torch.float32))
    assert not torch.equal(E.expect(tmut["db"], torch.float32), E.expect(tref["db"], torch.float32))


def test_mutations_linear():
    M, K, N = 4133, 60, 60
    op = E.linear_operands(M, K, N, "int", E.ACT_NONE, 1000)
    gy = E.dense_gy((M, N), 1005)
    ref = E.linear_ref(op["x"], op["w"], op["b"], op["res"], gy, None, E.ACT_NONE, 0.5)
    x, w = op["x"].double(), op["w"].double()
    names = ("token", "channel")
    m1 = ref["y"].clone()                                 # one term of one dot product dropped
    m1[M - 1, N - 1] -= 0.5 * x[M - 1, K - 1] * w[N - 1, K - 1]
    assert x[M - 1, K - 1] * w[N - 1, K - 1] != 0
    m2 = ref["y"].clone()                                 # two channels of one 8-channel chunk swapped in one row
    m2[2000, [17, 18]] = ref["y"][2000, [18, 17]]
    m3 = ref["y"].clone()                                 # the first row of a 32-token tile takes its neighbour's 8-channel chunk
    m3[32 * 40, 8:16] = ref["y"][32 * 40 + 1, 8:16]
    for i, m in enumerate((m1, m2, m3)):
        assert _exact_fires(m, ref["y"], names), f"mutation {i + 1}: the exact comparison did not fire"
        assert _gate_silent(m, ref["y"]), f"mutation {i + 1}: the relative-L2 gate fired"
    m4 = ref["dw"] - 0.5 * torch.outer(gy[M - 1].double(), x[M - 1])      # the last token lost from dW
    assert not torch.equal(m4.float(), ref["dw"].float()) and _gate_silent(m4, ref["dw"])
    gt, rows = E.linear_thin_gy(op["x"], N, 1006, E.LIMIT_BF16)
    assert M - 1 in rows.tolist()
    tref = E.linear_ref(op["x"], op["w"], None, None, gt, None, E.ACT_NONE, 0.5)
    tm = tref["dw"] - 0.5 * torch.outer(gt[M - 1].double(), x[M - 1])
    assert not torch.equal(E.expect(tm, torch.float32), E.expect(tref["dw"], torch.float32))
