"""Operands and float64 references for the exact-result tests (test_exact_host.py, test_exact_gpu.py): Linear without a
LayerNorm, the convolutions on rows (with PixelShuffle) and window attention with hard (0 or 2^-k) weights.  Plain torch in
float64 on the CPU; nothing here touches the code under test.

The idea: small integers and dyadic fractions are bf16-representable, their products are exact in fp32, and a sum of them is
exact in fp32 IN EVERY ORDER while the sum of the absolute values stays below 2^24 quanta (below 2^8 = 256 where a partial
sum is stored as bf16).  A kernel that drops, repeats or misplaces one term is then off by at least one quantum, and the
comparison is ``torch.equal``.  The rules the operands have to keep (R1 - R3, checked by `check_rules`):

  R1  every operand is bf16-representable (fp32x3: one operand may carry 16 significant bits, hi + lo), scales are powers
      of two;
  R2  sum |a||b| (+ |bias| + |residual|), in quanta of the operands, is below 2^24 for every output element;
  R3  where an output passes through bf16 partial sums, its absolute sum is at most 256 quanta.

A power-of-two scale changes the exponent of a sum and not its significand, so R2 and R3 are computed on the unscaled sums.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import rdst_oracle as O

ACT_NONE, ACT_LEAKY02 = 0, 2
LO_Q = 2.0 ** -9          # the quantum of a hi + lo operand (`hilo`)
LIMIT_F32, LIMIT_BF16 = float(2 ** 24), 256.0


# ---------------------------------------------------------------------------------------------------------------------
# operand generators (numpy PCG64, like util.rand)
# ---------------------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def ints(shape, seed, lo, hi):
    """Integers in [lo, hi] as fp32."""
    return torch.from_numpy(_rng(seed).integers(lo, hi + 1, size=shape).astype(np.float32))


def pos_ints(shape, seed, hi):
    """Strictly positive integers in [1, hi]: LeakyReLU and its derivative are the identity on them."""
    return ints(shape, seed, 1, hi)


def hilo(shape, seed, positive=False):
    """Values with 16 significant bits at most whose bf16 split has two nonzero terms: +-(h + m 2^-9), h and m in 1..3.
    bf16 keeps 8 bits, so hi = bf16(v) is h (or h + 2^-7) and lo = v - hi is a nonzero multiple of 2^-9 that bf16 holds."""
    g = _rng(seed)
    v = g.integers(1, 4, size=shape) + g.integers(1, 4, size=shape) * LO_Q
    if not positive:
        v = v * (2 * g.integers(0, 2, size=shape) - 1)
    return torch.from_numpy(v.astype(np.float32))


def split_hilo(v):
    """(hi, lo) of the two-term bf16 split of an fp32 tensor, as fp32."""
    hi = v.bfloat16().float()
    return hi, v - hi


def is_bf16(t):
    return bool(torch.equal(t.float().bfloat16().float(), t.float()))


def is_pow2(s):
    m, _ = np.frexp(float(s))
    return s > 0 and m == 0.5


def thin_rows(n_rows, rows_per_image, channels, seed, contrib, limit, cap=8192):
    """A thinned upstream gradient (n_rows, channels) with values in {-1, 0, 1}: nonzero on a random subset of the rows
    (tokens or pixels), the first and the last row of every image always among them (+-1 in every channel there), and the
    subset as large as `limit` allows.

    `contrib(idx)` gives, for the dY rows `idx`, the (len(idx), E) float64 matrix of what one unit of |dY| in that row adds
    to the absolute sum of each of E output elements (|x| of the row for a Linear, |x| of the 3 x 3 patch for a conv; a
    column of ones stands for dbias).  The rows are taken in a fixed order - the forced ones, then a random permutation of
    the others, `cap` rows at most - and the longest prefix whose running column sums all stay <= `limit` is kept.
    Returns (dY fp32, the sorted row indices)."""
    g = _rng(seed)
    n_img = n_rows // rows_per_image
    assert n_img * rows_per_image == n_rows
    first = np.arange(n_img) * rows_per_image
    forced = np.unique(np.concatenate([first, first + rows_per_image - 1]))
    rest = np.setdiff1d(np.arange(n_rows), forced)
    order = np.concatenate([forced, g.permutation(rest)])[:max(cap, len(forced))]
    cum = torch.cumsum(contrib(torch.from_numpy(order)).double(), 0).amax(1)
    keep = int((cum <= limit).sum())
    assert keep >= len(forced), f"thin_rows: the {len(forced)} forced rows alone exceed the limit {limit} ({cum[len(forced) - 1]})"
    rows = np.sort(order[:keep])
    dy = np.zeros((n_rows, channels), dtype=np.float32)
    dy[rows] = g.integers(-1, 2, size=(keep, channels))
    dy[forced] = 2 * g.integers(0, 2, size=(len(forced), channels)) - 1
    return torch.from_numpy(dy), torch.from_numpy(rows)


# ---------------------------------------------------------------------------------------------------------------------
# what a kernel is expected to return, and where it differs
# ---------------------------------------------------------------------------------------------------------------------
def expect(exact, dtype):
    """The float64 result in the kernel's output type: fp32 - the cast (exact by R2); bf16 - one round-to-nearest-even of
    it, which is what the epilogues do ((acc + b) * s + R in fp32, then from_f32)."""
    f = exact.to(torch.float32)
    assert torch.equal(f.double(), exact.double()), "expect: the float64 result is not an fp32 number (R2 does not hold)"
    return f.bfloat16() if dtype == torch.bfloat16 else f


def first_mismatches(got, want, names, limit=5):
    """The coordinates of the first few elements at which `got` and `want` differ, as text: `names` labels the dimensions
    ("image", "row", "column", "channel").  Empty when the tensors are equal."""
    got, want = got.detach().cpu(), want.detach().cpu()
    if got.shape != want.shape:
        return [f"shapes differ: got {tuple(got.shape)}, want {tuple(want.shape)}"]
    bad = (got != want) | (got != got)
    idx = bad.nonzero()
    out = []
    for row in idx[:limit].tolist():
        where = ", ".join(f"{n}={i}" for n, i in zip(names, row))
        out.append(f"({where}): got {got[tuple(row)].item()!r}, want {want[tuple(row)].item()!r}")
    if len(idx) > limit:
        out.append(f"... {len(idx)} of {got.numel()} elements differ")
    return out


def assert_equal(got, want, names, what):
    """torch.equal, with the place of the first misses in the message."""
    bad = first_mismatches(got, want, names)
    assert not bad, f"{what}: " + "; ".join(bad)


def bf16_half_ulp(exact):
    """Half a bf16 unit in the last place of each float64 value (0 at 0): 2^(e - 9) for |x| in [2^(e-1), 2^e)."""
    _, e = torch.frexp(exact.double())
    one = torch.ones_like(exact, dtype=torch.float64)
    return torch.where(exact == 0, 0 * one, torch.ldexp(one, e - 9))


# ---------------------------------------------------------------------------------------------------------------------
# Linear: Y = (act(X) W^T + b) * s + R;  dX = dX_add + act'(X) (s dY W);  dW = s dY^T act(X);  dbias = s sum dY
# ---------------------------------------------------------------------------------------------------------------------
def linear_ref(x, w, b, res, gy, add, act, scale):
    """float64, written out (no autograd).  act is identity, or LeakyReLU on strictly positive x (asserted): identity too."""
    if act != ACT_NONE:
        assert act == ACT_LEAKY02 and bool((x > 0).all()), "LeakyReLU cases take strictly positive inputs"
    x, w, gy = x.double(), w.double(), gy.double()
    y = x @ w.t()
    if b is not None:
        y = y + b.double()
    y = y * scale
    if res is not None:
        y = y + res.double()
    g = gy * scale
    dx = g @ w
    if add is not None:
        dx = dx + add.double()
    return {"y": y, "dx": dx, "dw": g.t() @ x, "db": g.sum(0)}


def quanta(config):
    """The quantum of each output: 2^-9 where the hi + lo operand enters it, 1 elsewhere (everything else is an integer)."""
    return {"y": 1.0 if config == "int" else LO_Q, "dx": LO_Q if config == "w_hilo" else 1.0,
            "dw": LO_Q if config == "x_hilo" else 1.0, "db": 1.0}


def linear_abs(x, w, b, res, gy, add, config="int"):
    """The absolute sums of R2 / R3 (unscaled, in quanta): the same formulas on the absolute values, maximum per output."""
    qs = quanta(config)
    r = linear_ref(x.abs(), w.abs(), None if b is None else b.abs(), None if res is None else res.abs(), gy.abs(),
                   None if add is None else add.abs(), ACT_NONE, 1.0)
    return {k: v.max().item() / qs[k] for k, v in r.items()}


def linear_contrib(x):
    """`contrib` of thin_rows for dW (|x| of the token) and dbias (one)."""
    ax = torch.cat([x.abs().double(), torch.ones(x.shape[0], 1, dtype=torch.float64)], 1)
    return lambda idx: ax[idx]


# ---------------------------------------------------------------------------------------------------------------------
# conv on rows: x (B, H, W, Cin), w (Cout, Cin, k, k), zero padding k // 2, * s, PixelShuffle(r), + R
# ---------------------------------------------------------------------------------------------------------------------
def conv_ref(x, w, b, res, gy, act, scale, r, want=("y", "dx", "dw", "db"), dtype=torch.float64):
    """float64 by torch autograd.  gy and res in the output geometry (B, H r, W r, Cout / r^2); dx token-major like x."""
    if act != ACT_NONE:
        assert act == ACT_LEAKY02 and bool((x > 0).all()), "LeakyReLU cases take strictly positive inputs"
    xr = x.to(dtype).clone().requires_grad_(True)
    wr = w.to(dtype).clone().requires_grad_(True)
    br = None if b is None else b.to(dtype).clone().requires_grad_(True)
    h = F.conv2d(xr.permute(0, 3, 1, 2), wr, br, padding=w.shape[-1] // 2)
    if r > 1:
        h = F.pixel_shuffle(h, r)
    y = h.permute(0, 2, 3, 1) * scale
    out = {}
    if any(k in want for k in ("dx", "dw", "db")):
        y.backward(gy.to(dtype))
        out = {"dx": xr.grad, "dw": wr.grad, "db": None if br is None else br.grad}
    y = y.detach()
    out["y"] = y if res is None else y + res.to(dtype)
    return out


ABS_MARGIN = 1.0 + 2.0 ** -10


def conv_abs(x, w, b, res, gy, r, config="int"):
    """The absolute sums of R2 / R3 (unscaled, in quanta).  Summed in fp32 (a float64 conv costs ten times as much): sums of
    nonnegative terms, so the fp32 result is within n 2^-24 < 2^-10 of the true one, and that margin is added."""
    r_ = conv_ref(x.abs(), w.abs(), None if b is None else b.abs(), None if res is None else res.abs(), gy.abs(), ACT_NONE, 1.0, r,
                  dtype=torch.float32)
    qs = quanta(config)
    return {k: v.max().item() * ABS_MARGIN / qs[k] for k, v in r_.items() if v is not None}


def _patches(x, pix, k):
    """(len(pix), k, k, Cin) float64: the k x k neighbourhood (zero padded) of the conv pixels `pix` (flat over B, H, W)."""
    B, H, W, Cin = x.shape
    p = k // 2
    xp = F.pad(x.double(), (0, 0, p, p, p, p))
    bi, yi, xi = pix // (H * W), (pix // W) % H, pix % W
    rows = [torch.stack([xp[bi, yi + ky, xi + kx] for kx in range(k)], 1) for ky in range(k)]
    return torch.stack(rows, 1)


def conv_contrib(x, k, r):
    """`contrib` of thin_rows for a conv: dY rows are pixels of the OUTPUT geometry (B, H r, W r); one unit there adds the
    |x| of the conv pixel's patch to dW (to the output channels of its sub-pixel only: the bound is on the safe side)."""
    B, H, W, Cin = x.shape
    ax = x.abs()

    def contrib(idx):
        yo, xo = (idx // (W * r)) % (H * r), idx % (W * r)
        pix = (idx // (H * r * W * r)) * (H * W) + (yo // r) * W + xo // r
        pt = _patches(ax, pix, k).reshape(len(idx), -1)
        return torch.cat([pt, torch.ones(len(idx), 1, dtype=torch.float64)], 1)
    return contrib


def conv_wgrad_sparse(x, gy, rows, Cout, k, scale, r):
    """dW and dbias in float64 for a dY that is zero outside the pixel rows `rows` (thin_rows): the sum over those pixels of
    dY (x) patch, written out - the same numbers as conv_ref's, at a fraction of the cost."""
    B, H, W, Cin = x.shape
    cy = Cout // (r * r)
    g = gy.reshape(-1, cy)[rows].double() * scale                      # (n, cy)
    yo, xo = (rows // (W * r)) % (H * r), rows % (W * r)
    pix = (rows // (H * r * W * r)) * (H * W) + (yo // r) * W + xo // r
    pt = _patches(x, pix, k)                                            # (n, k, k, Cin)
    sub = (yo % r) * r + xo % r                                         # conv channel = c' r^2 + sub (PixelShuffle)
    dw = torch.zeros(cy, r * r, Cin, k, k, dtype=torch.float64)
    db = torch.zeros(cy, r * r, dtype=torch.float64)
    for q in range(r * r):
        m = sub == q
        if bool(m.any()):
            dw[:, q] = torch.einsum("nc,nyxi->ciyx", g[m], pt[m])
            db[:, q] = g[m].sum(0)
    return {"dw": dw.reshape(Cout, Cin, k, k), "db": db.reshape(Cout)}


# ---------------------------------------------------------------------------------------------------------------------
# window attention with hard weights: q = 0, so the logits are the bias table (+ the shift mask)
# ---------------------------------------------------------------------------------------------------------------------
TABLES = ("zero", "centre", "probe")


def attn_table(kind, ws, heads, seed):
    """zero: uniform weights over a window (a mask region under a shift); centre: -100 everywhere but the centre offset
    (identity weights); probe: -100 everywhere but ONE random offset per head (shift 0 only: each row has that partner, or
    none and falls back to 1 / N)."""
    T = (2 * ws - 1) ** 2
    if kind == "zero":
        return torch.zeros(T, heads)
    t = torch.full((T, heads), -100.0)
    centre = (ws - 1) * (2 * ws - 1) + (ws - 1)
    if kind == "centre":
        t[centre] = 0.0
    elif kind == "probe":
        g = _rng(seed)
        for h in range(heads):
            t[int(g.integers(0, T)), h] = 0.0
    else:
        raise ValueError(kind)
    return t


def attn_operands(B, H, W, C, seed):
    """qkv with a zero q part and small-integer k and v of different ranges (a q / k / v slot mix-up shows), integer dO."""
    qkv = torch.zeros(B, H, W, 3 * C)
    qkv[..., C:2 * C] = ints((B, H, W, C), seed, -7, 7)
    qkv[..., 2 * C:] = ints((B, H, W, C), seed + 1, -3, 3)
    return qkv, ints((B, H, W, C), seed + 2, -3, 3)


def attn_weights(table, H, W, heads, ws, shift):
    """The float64 softmax of (bias + mask), (nW, heads, N, N), as the oracle forms it."""
    N = ws * ws
    idx = O.relative_position_index(ws).reshape(-1)
    logits = table.double()[idx].reshape(N, N, heads).permute(2, 0, 1)[None]
    if shift > 0:
        logits = logits + O.calculate_mask(H, W, ws, shift, dtype=torch.float64)[:, None]
    else:
        logits = logits.expand((H // ws) * (W // ws), heads, N, N)
    return torch.softmax(logits, dim=-1)


def harden(P):
    """(hard weights, the largest |P - hard|): every weight below 1e-30 becomes 0, every other the nearest power of two."""
    hard = torch.where(P < 1e-30, torch.zeros_like(P), torch.exp2(torch.round(torch.log2(P.clamp_min(1e-300)))))
    return hard, (P - hard).abs().max().item()


def attn_ref(qkv, table, dO, heads, ws, shift, scale):
    """float64 results of window attention at HARD weights: {"o", "dv", "abs_o", "abs_dv", "soft_o", "dev"} - o (B, H, W, C),
    dv the v third of d(qkv), abs_* = sum_j P |v| (the scale of the rounding bounds), soft_o the oracle's own output with
    the -100 logits left soft (their leak is exp(-100)), dev = how far the soft weights are from 0 / 2^-k."""
    B, H, W, C3 = qkv.shape
    C, N = C3 // 3, ws * ws
    d = C // heads
    assert bool((qkv[..., :C] == 0).all()), "the q part must be zero"
    hard, dev = harden(attn_weights(table, H, W, heads, ws, shift))
    nW = hard.shape[0]

    def apply(v, Pm):        # v (B, H, W, C) -> (B, H, W, C), roll / partition / reverse as the oracle does
        if shift > 0:
            v = torch.roll(v, shifts=(-shift, -shift), dims=(1, 2))
        vw = O.window_partition(v, ws).reshape(B, nW, N, heads, d).permute(0, 1, 3, 2, 4)
        o = (Pm[None] @ vw).permute(0, 1, 3, 2, 4).reshape(-1, ws, ws, C)
        o = O.window_reverse(o, ws, H, W)
        return torch.roll(o, shifts=(shift, shift), dims=(1, 2)) if shift > 0 else o

    v = qkv[..., 2 * C:].double().clone().requires_grad_(True)
    o = apply(v, hard)
    o.backward(dO.double())
    va = qkv[..., 2 * C:].double().abs().clone().requires_grad_(True)
    oa = apply(va, hard)
    oa.backward(dO.double().abs())
    soft = O.window_attention_core(qkv.double(), table.double(), heads, ws, shift, scale)
    return {"o": o.detach(), "dv": v.grad, "abs_o": oa.detach(), "abs_dv": va.grad, "soft_o": soft, "dev": dev}


@functools.lru_cache(maxsize=None)
def attn_case(B, H, W, C, heads, ws, shift, kind, seed=1):
    """One seeded attention case with its reference, computed once and read only."""
    qkv, dO = attn_operands(B, H, W, C, 100 * seed + 7)
    table = attn_table(kind, ws, heads, 100 * seed + 11)
    ref = attn_ref(qkv, table, dO, heads, ws, shift, 0.25)
    return {"qkv": qkv, "dO": dO, "table": table, **ref}


# ---------------------------------------------------------------------------------------------------------------------
# The cases and draws of test_exact_gpu.py (test_exact_host.py checks every one of them on the CPU)
# ---------------------------------------------------------------------------------------------------------------------
MODES = ("f32", "bf16", "f32x3")
# which operand carries hi + lo: none (every operand bf16-exact) in fp32 and bf16; in fp32x3 first x, then the weight - the
# other operand of each product is bf16-exact, so the three-term product is exact and each lo term is under test
CONFIGS = {"f32": ("int",), "bf16": ("int",), "f32x3": ("x_hilo", "w_hilo")}


def pow2_scale(s):
    """The scales of the existing case lists, as powers of two."""
    return {0.7: 0.5, 0.9: 0.25}.get(s, s)


# (M, K, N) of LIN in test_ops_gpu.py, then (K, N) of SHAPES in test_lnlin3_gpu.py at M = 1189 and 4133
LINEAR_SHAPES = [(256, 60, 180), (256, 60, 60), (200, 90, 180), (256, 180, 90), (192, 120, 30), (288, 120, 30), (160, 90, 270),
                 (130, 48, 48), (4133, 60, 60), (64, 33, 17), (384, 90, 270), (320, 240, 120), (416, 120, 240)]
LINEAR_SHAPES += [(M, K, N) for M in (1189, 4133)
                  for K, N in ((60, 180), (90, 270), (120, 360), (60, 60), (90, 90), (120, 120), (60, 30), (90, 30), (120, 30))
                  if (M, K, N) not in LINEAR_SHAPES]
# through ops.ln_linear: (bias, residual, out_scale, in_act)
LINEAR_VARIANTS = [(False, False, 1.0, ACT_NONE), (True, True, 0.5, ACT_LEAKY02), (True, False, 0.25, ACT_NONE)]
# through rdst_ln_linear_bwd: (in_act, out_scale, dX_add)
LINEAR_BWD_VARIANTS = [(ACT_NONE, 1.0, False), (ACT_NONE, 1.0, True), (ACT_LEAKY02, 0.5, True)]


def linear_operands(M, K, N, config, act, seed):
    """{"x", "w", "b", "res", "add"}: integers, the hi + lo operand per `config`, x strictly positive behind a LeakyReLU."""
    pos = act != ACT_NONE
    if config == "x_hilo":
        x = hilo((M, K), seed, positive=pos)
    else:
        x = pos_ints((M, K), seed, 3) if pos else ints((M, K), seed, -3, 3)
    w = hilo((N, K), seed + 1) if config == "w_hilo" else ints((N, K), seed + 1, -2, 2)
    return {"x": x, "w": w, "b": ints((N,), seed + 2, -4, 4), "res": ints((M, N), seed + 3, -8, 8),
            "add": ints((M, K), seed + 4, -8, 8)}


def dense_gy(shape, seed):
    return ints(shape, seed, -2, 2)


def linear_thin_gy(x, N, seed, limit):
    """(dY, rows): `limit` in the units of x (256 for bf16 partials, 2^24 quanta for an fp32 sum)."""
    return thin_rows(x.shape[0], x.shape[0], N, seed, linear_contrib(x), limit)


def linear_draws(op, N, mode, config, seed):
    """[(name, dY, thinned rows or None, outputs asserted on it)]: bf16 - y and dX on the dense draw, everything on the thinned
    one (R3); fp32 / fp32x3 - everything on the dense draw, unless its dW breaks R2 (then as bf16, thinned to 2^24 quanta)."""
    q = quanta(config)["dw"]
    gy = dense_gy((op["x"].shape[0], N), seed + 5)
    dense_dw = linear_abs(op["x"], op["w"], None, None, gy, None, config)["dw"]
    if mode != "bf16" and dense_dw < LIMIT_F32:
        return [("dense", gy, None, ("y", "dx", "dw", "db"))]
    limit = LIMIT_BF16 if mode == "bf16" else (LIMIT_F32 - 1) * q
    gt, rows = linear_thin_gy(op["x"], N, seed + 6, limit)
    return [("dense", gy, None, ("y", "dx")), ("thin", gt, rows, ("y", "dx", "dw", "db"))]


# B, H, W, Cin, Cout, k, act, residual, scale, shuffle: CONV of test_ops_gpu.py with power-of-two scales
CONV_CASES = [
    (2, 8, 8, 150, 60, 3, 0, True, 0.5, 1), (1, 8, 12, 60, 240, 3, 0, False, 1.0, 2), (2, 9, 7, 1, 60, 3, 0, False, 1.0, 1),
    (1, 16, 16, 60, 1, 3, 0, False, 1.0, 1), (2, 24, 40, 60, 1, 3, 0, False, 0.5, 1), (1, 9, 11, 36, 1, 3, 0, False, 1.0, 1),
    (2, 6, 6, 37, 12, 1, 2, False, 1.0, 1), (1, 6, 6, 48, 108, 3, 0, False, 1.0, 3), (2, 5, 5, 3, 3, 1, 0, False, 1.0, 1),
    (2, 16, 25, 1, 1, 1, 0, True, 0.5, 1), (1, 7, 9, 1, 1, 1, 0, True, 1.0, 1), (1, 8, 32, 150, 60, 3, 0, True, 0.5, 1),
    (1, 4, 32, 60, 240, 3, 0, False, 1.0, 2), (1, 6, 10, 150, 60, 3, 2, True, 1.0, 1),
    (33, 6, 256, 150, 60, 3, 0, True, 0.5, 1), (33, 6, 256, 60, 60, 3, 0, True, 0.5, 1), (33, 6, 256, 60, 240, 3, 0, False, 1.0, 2),
]
# B, H, W, Cout, scale of test_head_conv_one_input_channel: one input channel, no gradient asked for x
HEAD_CONV_CASES = [(2, 9, 7, 60, 1.0), (3, 40, 70, 60, 0.5), (1, 16, 16, 36, 1.0)]
LARGE_PIXELS = 33 * 6 * 256          # from here on the thinned draw is repeated with three seeds


def thin_seeds(B, H, W):
    return (0, 1, 2) if B * H * W >= LARGE_PIXELS else (0,)


def conv_operands(B, H, W, Cin, Cout, k, act, r, config, seed):
    pos = act != ACT_NONE
    if config == "x_hilo":
        x = hilo((B, H, W, Cin), seed, positive=pos)
    else:
        x = pos_ints((B, H, W, Cin), seed, 3) if pos else ints((B, H, W, Cin), seed, -3, 3)
    w = hilo((Cout, Cin, k, k), seed + 1) if config == "w_hilo" else ints((Cout, Cin, k, k), seed + 1, -2, 2)
    cy = Cout // (r * r)
    return {"x": x, "w": w, "b": ints((Cout,), seed + 2, -4, 4), "res": ints((B, H * r, W * r, cy), seed + 3, -8, 8)}


def conv_thin_gy(x, Cout, k, r, seed, limit):
    """(dY in the output geometry, pixel rows)."""
    B, H, W, _ = x.shape
    cy = Cout // (r * r)
    gy, rows = thin_rows(B * H * r * W * r, H * r * W * r, cy, seed, conv_contrib(x, k, r), limit)
    return gy.reshape(B, H * r, W * r, cy), rows


def conv_dense_asserted(mode, bounds, x_grad=True):
    """(the outputs asserted on the dense draw, whether dW / dbias are among them): bf16 - y and dX only (R3: dW and dbias take
    thinned draws); fp32 / fp32x3 - everything, unless the dense dW breaks R2."""
    dense_w = mode != "bf16" and bounds["dw"] < LIMIT_F32
    return [k for k in (("y", "dx", "dw", "db") if dense_w else ("y", "dx")) if x_grad or k != "dx"], dense_w


def conv_thin_limit(mode, config):
    """In the units of x: 256 behind bf16 partials, else 2^24 quanta."""
    return LIMIT_BF16 if mode == "bf16" else (LIMIT_F32 - 1) * quanta(config)["dw"]


def check_rules(operands, hilo_name, scale, bounds, asserted, mode):
    """R1 - R3 as assertions.  `operands`: name -> tensor (None allowed); `hilo_name`: the one operand that may carry 16
    bits; `bounds`: the absolute sums in quanta; `asserted`: the outputs this draw is compared on."""
    for name, t in operands.items():
        if t is None:
            continue
        if name == hilo_name:
            hi, lo = split_hilo(t)
            assert bool((hi != 0).all()) and bool((lo != 0).all()), f"R1: {name} needs two nonzero terms"
            assert is_bf16(hi) and is_bf16(lo) and torch.equal(hi + lo, t), f"R1: {name} is not hi + lo of two bf16 numbers"
        else:
            assert is_bf16(t), f"R1: {name} is not bf16-representable"
    assert is_pow2(scale), f"R1: the scale {scale} is not a power of two"
    for k in asserted:
        assert bounds[k] < LIMIT_F32, f"R2: the absolute sum of {k} is {bounds[k]:.0f} quanta >= 2^24"
        if mode == "bf16" and k in ("dw", "db"):
            assert bounds[k] <= LIMIT_BF16, f"R3: the absolute sum of {k} is {bounds[k]:.0f} > 256 behind bf16 partials"


# B, H, W, C, heads, ws, shift: the shapes of CASES, BF16_ROUTE_CASES and WS16_CASES of test_wattn_gpu.py (dyadic shifts only)
ATTN_CASES = [
    (2, 16, 16, 60, 6, 8, 0), (2, 16, 16, 60, 6, 8, 4),
    (1, 16, 24, 90, 6, 8, 0), (1, 16, 24, 90, 6, 8, 4),       # non-square, head dim 15
    (1, 24, 16, 120, 6, 8, 0), (1, 24, 16, 120, 6, 8, 4),     # head dim 20
    (3, 8, 8, 48, 6, 8, 0), (1, 8, 16, 48, 6, 8, 4),          # head dim 8
    (2, 8, 8, 60, 6, 8, 4),                                   # shifted, one window per image
    (1, 8, 16, 60, 3, 8, 0), (1, 8, 16, 60, 3, 8, 4),         # the 3-head route
    (2, 8, 12, 72, 6, 4, 2), (1, 8, 16, 48, 6, 4, 2),         # window 4
    (1, 32, 32, 60, 6, 16, 0), (1, 32, 32, 60, 6, 16, 8), (1, 32, 48, 90, 6, 16, 8), (2, 48, 32, 120, 6, 16, 8),
    (1, 32, 48, 48, 6, 16, 0),
]
ATTN_RUNS = [(*c, kind) for c in ATTN_CASES for kind in TABLES if kind != "probe" or c[6] == 0]


def assert_within(got, exact, tol, names, what):
    """|got - exact| <= tol elementwise (tol a float64 tensor or a number), with the place of the first misses in the message."""
    got = got.detach().double().cpu()
    tol = tol if torch.is_tensor(tol) else torch.full_like(exact, float(tol))
    bad = ~((got - exact).abs() <= tol)
    if bool(bad.any()):
        idx = bad.nonzero()
        msg = []
        for row in idx[:5].tolist():
            where = ", ".join(f"{n}={i}" for n, i in zip(names, row))
            t = tuple(row)
            msg.append(f"({where}): got {got[t].item()!r}, exact {exact[t].item()!r}, allowed {tol[t].item():.3e}")
        raise AssertionError(f"{what}: {len(idx)} of {got.numel()} elements off; " + "; ".join(msg))
