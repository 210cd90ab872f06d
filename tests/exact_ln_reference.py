"""Operands and float64 references for the exact-result tests of LayerNorm, GELU and the fused Mlp (test_exact_ln_host.py,
test_exact_ln_gpu.py).  It continues exact_reference.py (rules R1 - R3, `expect`, `assert_equal`, `thin_rows`); plain torch in
float64 on the CPU, nothing here touches the code under test.

Hard LayerNorm rows.  Row r is x = m_r + s_r sigma_r with sigma_r a balanced vector of +-1 (C is even), m_r an integer and
s_r a power of two: the row mean is m_r and the variance s_r^2, both as exact integer sums in every order, and
x-hat = (x - m_r) / s_r = sigma_r.  With gamma in {1/2, 1, 2} and beta in {-1, 0, 1} the LayerNorm output z = gamma sigma + beta
is a small dyadic number.  What eps = 1e-5 does to this: the true x-hat is sigma s / sqrt(s^2 + eps) = sigma (1 - eps / (2 s^2) + ...),
5e-6 away from +-1 at s = 1 and 1.2e-9 at s = 64.  So every case carries TWO float64 evaluations:

  hard   x-hat = sigma and rstd = 1 / s, GELU = max(h, 0), GELU' in {0, 1/2, 1}, written out without autograd: sums of dyadic
         products, exact in float64 and (R2) in fp32 - what the kernels are compared with (`torch.equal`);
  true   torch autograd in float64 through F.layer_norm (eps 1e-5) and the erf GELU of the oracle: the definition.  The host
         tests assert |true - hard| <= LEAK(s_min) A per output element, A the absolute sum of that element, LEAK = 2 eps / s^2
         (two factors of x-hat / rstd at most enter any term; the GELU part leaks Phi(-16) < 1e-57).  Without a LayerNorm
         (the GELU Linear) true and hard agree to 1e-9 of a quantum.

Hard GELU.  Every pre-activation h is a multiple of 16: GELU(0) = 0 and GELU'(0) = 1/2; at |h| >= 16 GELU = max(h, 0) and GELU'
is 0 or 1 in fp32 on every route (see test_exact_ln_gpu.py).

The LayerNorm backward dX = rstd (g - mean(g) - x-hat mean(g x-hat)) (+ addend) divides by C and is not exact: `ln_dx` returns
it in float64 for the rstd the kernel is handed (or forms) together with A, the absolute sum of its terms; the tests bound the
kernel's error by 1/2 ulp_bf16 + ((1 + 2^-24)^n - 1) A.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import exact_reference as E
from oracle import rdst_oracle as O

ACT_NONE, ACT_GELU = 0, 1
LN_EPS = 1e-5
GELU_Q = 16.0            # the quantum of a hard pre-activation
U24 = 2.0 ** -24


def leak(s_min):
    """How far eps moves a LayerNorm result, relative to its absolute sum (see the module docstring)."""
    return 2.0 * LN_EPS / float(s_min) ** 2


def roundings(n):
    """(1 + 2^-24)^n - 1: what n fp32 roundings in a row can do to a term."""
    return (1.0 + U24) ** n - 1.0


# ---------------------------------------------------------------------------------------------------------------------
# float32 emulation of the row statistics, as the kernels form them
# ---------------------------------------------------------------------------------------------------------------------
STAT_ROUTES = ("div", "mul", "fma")


def _rstd32(var_f32=None, fused=None):
    """1 / sqrtf(var + eps) in float32; `fused` = (sq, inv): var * inv + eps contracted into ONE fma (one rounding)."""
    if fused is not None:
        sq, inv = fused
        arg = (sq.astype(np.float64) * np.float64(inv) + np.float64(np.float32(LN_EPS))).astype(np.float32)   # 48 + 24 bits: exact in float64 here
    else:
        arg = var_f32 + np.float32(LN_EPS)
    return np.float32(1.0) / np.sqrt(arg, dtype=np.float32)


def emulate_stats(x, route):
    """(mean, rstd) in float32 arithmetic for rows whose sums are exact (asserted), by the formula of the route, read from the
    code: `div` - row_stats_kernel of linear.hip (sum / (float)K, sum of (x - mean)^2 / (float)K, 1 / sqrtf(var + eps)); `mul` -
    the kernels that multiply by fl(1 / K) (linear_mfma.hip:290-303, mlp_mfma.hip:781-793), every operation rounded; `fma` - the
    same as the compiler emits it: var * invK + eps contracted into one fused multiply-add (measured on the device: with
    K fl(1 / K) = 1 + 0.44 * 2^-23 at K = 60 the contracted argument of s = 8 rounds two ulps above 64 and rstd comes out one ulp
    below 1 / 8)."""
    K = x.shape[1]
    xs = x.double()
    assert float(xs.abs().sum(1).max()) < 2 ** 24, "the row sum is not exact in fp32"
    sums = xs.sum(1).numpy().astype(np.float32)
    kf = np.float32(K)
    inv = np.float32(1.0) / kf
    mean = sums / kf if route == "div" else sums * inv
    d = xs.numpy() - mean.astype(np.float64)[:, None]
    sq = (d * d).sum(1)
    assert float(sq.max()) < 2 ** 24 and np.array_equal(sq, np.round(sq * 4096) / 4096), "the sum of squares is not exact in fp32"
    sq = sq.astype(np.float32)
    rstd = _rstd32(fused=(sq, inv)) if route == "fma" else _rstd32(sq / kf if route == "div" else sq * inv)
    return torch.from_numpy(mean.astype(np.float32)), torch.from_numpy(rstd.astype(np.float32))


@functools.lru_cache(maxsize=None)
def exact_means(K, bound=256):
    """The integers m, |m| <= bound, whose mean comes out exact on every route: fl(fl(K m) fl(1 / K)) == m."""
    kf = np.float32(K)
    inv = np.float32(1.0) / kf
    m = np.arange(-bound, bound + 1).astype(np.float32)
    ok = ((m * kf) * inv == m) & ((m * kf) / kf == m)
    return m[ok].astype(np.int64)


def exact_scales(K, mode):
    """The powers of two s in 8 .. 128 whose rstd is exactly 1 / s on every route (fp32 / fp32x3: nothing narrows, so it has to
    be; s = 8 fails under the contracted formula at K = 60, 90, 120); bf16 adds s = 1 and 2, where s rstd is 5e-6 / 1.3e-6 below
    1 and the kernels that form x-hat narrow it to bf16, i.e. to +-1 exactly."""
    kf = np.float32(K)
    inv = np.float32(1.0) / kf
    out = []
    for s in (8, 16, 32, 64, 128):
        sq = np.array([K * s * s], dtype=np.float32)
        r = [_rstd32(sq / kf), _rstd32(sq * inv), _rstd32(fused=(sq, inv))]
        if all(v[0] == np.float32(1.0 / s) for v in r):
            out.append(s)
    return ([1, 2] if mode == "bf16" else []) + out


# ---------------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------------
def ln_rows(M, C, mode, seed):
    """{"x" (M, C) fp32, "m" (M), "s" (M), "sigma" (M, C)}: hard rows.  Rows 0 and 1 - and the rows on either side of every
    32-token tile border that exists - share their pattern and scale and differ only in m (statistics taken from the
    neighbouring token then show); rows 2 and M - 1 have s = 64, row 0 has s = 16; row 3 has the smallest scale of the mode (s = 1 in bf16).  In bf16 every element
    m +- s is bf16-representable."""
    assert C % 2 == 0
    g = E._rng(seed)
    means, scales = exact_means(C), exact_scales(C, mode)
    assert 64 in scales and (mode != "bf16" or 1 in scales)

    def fitting(s):        # the means that go with the scale s
        if mode != "bf16":
            return means
        lo, hi = torch.from_numpy((means - s).astype(np.float32)), torch.from_numpy((means + s).astype(np.float32))
        ok = (lo.bfloat16().float() == lo) & (hi.bfloat16().float() == hi)
        return means[ok.numpy()]

    fit = {s: fitting(s) for s in scales}
    assert all(len(v) > 8 for v in fit.values())

    def draw_m(s, avoid=None):
        for _ in range(1000):
            m = int(fit[s][g.integers(0, len(fit[s]))])
            if m != avoid:
                return m
        raise AssertionError("ln_rows: no mean fits")

    s = np.array([scales[i] for i in g.integers(0, len(scales), size=M)], dtype=np.int64)
    if M > 2:
        s[2] = 64
    if M > 3:
        s[3] = scales[0]
    s[0] = 16          # the first and the last row keep their gradient on every thinned draw (thin8 drops rows of s < 8)
    if M > 4:
        s[M - 1] = 64
    sigma = np.ones((M, C), dtype=np.int64)
    sigma[:, C // 2:] = -1
    sigma = g.permuted(sigma, axis=1)
    m = np.zeros(M, dtype=np.int64)
    for sc in scales:
        at = np.nonzero(s == sc)[0]
        m[at] = fit[sc][g.integers(0, len(fit[sc]), size=len(at))]
    pairs = [(0, 1)] + [(t - 1, t) for t in range(32, M, 32)]
    for a, b in pairs:
        if b < M and b != 2 and b != 3:
            s[b] = s[a]
            sigma[b] = sigma[a]
            m[b] = draw_m(int(s[a]), avoid=int(m[a]))
    x = m[:, None] + s[:, None] * sigma
    out = {"x": torch.from_numpy(x.astype(np.float32)), "m": torch.from_numpy(m).double(), "s": torch.from_numpy(s).double(),
           "sigma": torch.from_numpy(sigma).double(), "pairs": [(a, b) for a, b in pairs if b < M and b not in (2, 3)]}
    return out


def ln_affine(C, seed):
    """gamma in {1/2, 1, 2} and beta in {-1, 0, 1}, every value present."""
    g = E._rng(seed)
    gamma = np.array([0.5, 1.0, 2.0])[g.integers(0, 3, size=C)]
    beta = g.integers(-1, 2, size=C).astype(np.float64)
    gamma[:3], beta[:3] = (0.5, 1.0, 2.0), (-1.0, 0.0, 1.0)
    return torch.from_numpy(gamma.astype(np.float32)), torch.from_numpy(beta.astype(np.float32))


def sparse_ints(shape, seed, nnz, hi=1):
    """Integers in [-hi, hi] with `nnz` nonzero entries per row (the last dimension), at random places."""
    g = E._rng(seed)
    rows, cols = shape
    out = np.zeros(shape, dtype=np.float32)
    for r in range(rows):
        n = int(nnz[r % len(nnz)]) if hasattr(nnz, "__len__") else int(nnz)
        idx = g.choice(cols, size=min(n, cols), replace=False)
        out[r, idx] = g.integers(1, hi + 1, size=len(idx)) * (2 * g.integers(0, 2, size=len(idx)) - 1)
    return torch.from_numpy(out)


def hard_h(shape, seed):
    """A hard pre-activation: multiples of 16 in [-48, 48], a third of them zero."""
    g = E._rng(seed)
    k = g.integers(1, 4, size=shape) * g.integers(-1, 2, size=shape)
    return torch.from_numpy((GELU_Q * k).astype(np.float32))


def class_shares(h):
    """The shares of h = 0, h >= 16 and h <= -16; every h must be in one of them."""
    n = h.numel()
    z, p, q = int((h == 0).sum()), int((h >= GELU_Q).sum()), int((h <= -GELU_Q).sum())
    assert z + p + q == n and torch.equal(h / GELU_Q, (h / GELU_Q).round()), "a pre-activation is not a multiple of 16"
    return z / n, p / n, q / n


def assert_classes(h, what):
    """Each class above 10 % of the entries, and present in (nearly) every row and every unit."""
    sh = class_shares(h)
    assert min(sh) > 0.10, f"{what}: class shares {sh}"
    for cls in ((h == 0), (h >= GELU_Q), (h <= -GELU_Q)):
        assert float(cls.any(0).double().mean()) > 0.9 or h.shape[0] < 16, f"{what}: a class is missing from many units"
        assert float(cls.any(1).double().mean()) > 0.9, f"{what}: a class is missing from many rows"


def hard_gelu(h):
    """(GELU, GELU') of a hard pre-activation, float64."""
    h = h.double()
    return h.clamp_min(0.0), torch.where(h == 0, torch.full_like(h, 0.5), (h > 0).double())


def gelu64(h):
    return O.gelu(h)


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm backward, written out
# ---------------------------------------------------------------------------------------------------------------------
def ln_dx(g, sigma, rstd, add=None):
    """(dX, A) in float64: dX = rstd (g - mean(g) - sigma mean(g sigma)) + add for x-hat = sigma, and the absolute sum of its
    terms A = rstd (|g| + |mean(g)| + |mean(g sigma)|) + |add|."""
    g, sigma, rstd = g.double(), sigma.double(), rstd.double().reshape(-1, 1)
    s1, s2 = g.mean(1, keepdim=True), (g * sigma).mean(1, keepdim=True)
    dx = rstd * (g - s1 - sigma * s2)
    A = rstd * (g.abs() + s1.abs() + s2.abs())
    if add is not None:
        dx, A = dx + add.double(), A + add.double().abs()
    return dx, A


def ln_dx_abs_halves(op, gy, sc, rstd, add=None):
    """A of `ln_dx` summed over the two halves of the output features, [0, N1) and [N1, N), N1 = ceil4(N / 2)."""
    N = op["w"].shape[0]
    N1 = (N // 2 + 3) // 4 * 4
    G, w = gy.double() * sc, op["w"].double()
    A = 0
    for lo, hi in ((0, N1), (N1, N)):
        g = (G[:, lo:hi] @ w[lo:hi]) * op["gamma"].double()
        A = A + ln_dx(g, op["rows"]["sigma"], rstd)[1]
    return A if add is None else A + add.double().abs()


def true_rstd(s):
    return 1.0 / torch.sqrt(s.double() ** 2 + LN_EPS)


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm + Linear: Y = (LN(X) W^T + b) sc + R
# ---------------------------------------------------------------------------------------------------------------------
def ln_linear_hard(rows, gamma, beta, w, b, res, gy, sc):
    """The hard evaluation, written out.  {"y", "dw", "db", "dlw", "dlb"} exact; "g" = dA gamma, the input of `ln_dx`."""
    sigma = rows["sigma"]
    z = gamma.double() * sigma + beta.double()
    y = z @ w.double().t()
    if b is not None:
        y = y + b.double()
    y = y * sc
    if res is not None:
        y = y + res.double()
    G = gy.double() * sc
    dA = G @ w.double()
    return {"y": y, "dw": G.t() @ z, "db": G.sum(0), "dlw": (dA * sigma).sum(0), "dlb": dA.sum(0), "g": dA * gamma.double(), "z": z}


def ln_linear_abs(rows, gamma, beta, w, b, res, gy):
    """The absolute sums of R2 / R3, unscaled, per output (maxima), in the output's own units."""
    az = gamma.double() * rows["sigma"].abs() + beta.double().abs()
    aw, ag = w.double().abs(), gy.double().abs()
    y = az @ aw.t() + (0 if b is None else b.double().abs()) + (0 if res is None else res.double().abs())
    dA = ag @ aw
    return {"y": y.max().item(), "dw": (ag.t() @ az).max().item(), "db": ag.sum(0).max().item(), "dlw": dA.sum(0).max().item(),
            "dlb": dA.sum(0).max().item(), "G": (ag.t() @ rows["sigma"].abs()).max().item(), "dA": dA.max().item()}


def ln_linear_true(x, gamma, beta, w, b, res, gy, sc, add=None, eps=LN_EPS):
    """The definition: float64 autograd through F.layer_norm (eps = 0: the limit the hard evaluation stands for)."""
    leaves = [None if t is None else t.double().clone().requires_grad_(True) for t in (x, gamma, beta, w, b)]
    xr, lw, lb, wr, br = leaves
    y = F.linear(F.layer_norm(xr, (x.shape[-1],), lw, lb, eps), wr, br) * sc
    y.backward(gy.double())
    y = y.detach()
    return {"y": y if res is None else y + res.double(), "dx": xr.grad if add is None else xr.grad + add.double(), "dw": wr.grad,
            "db": None if br is None else br.grad, "dlw": lw.grad, "dlb": lb.grad}


# ---------------------------------------------------------------------------------------------------------------------
# GELU + Linear: Y = (GELU(H) W^T + b) sc + R
# ---------------------------------------------------------------------------------------------------------------------
def gelu_linear_hard(h, w, b, res, gy, add, sc):
    a, d = hard_gelu(h)
    y = a @ w.double().t()
    if b is not None:
        y = y + b.double()
    y = y * sc
    if res is not None:
        y = y + res.double()
    G = gy.double() * sc
    dx = d * (G @ w.double())
    if add is not None:
        dx = dx + add.double()
    return {"y": y, "dx": dx, "dw": G.t() @ a, "db": G.sum(0)}


def gelu_linear_true(h, w, b, res, gy, add, sc):
    hr, wr = h.double().clone().requires_grad_(True), w.double().clone().requires_grad_(True)
    br = None if b is None else b.double().clone().requires_grad_(True)
    y = F.linear(gelu64(hr), wr, br) * sc
    y.backward(gy.double())
    y = y.detach()
    return {"y": y if res is None else y + res.double(), "dx": hr.grad if add is None else hr.grad + add.double(), "dw": wr.grad,
            "db": None if br is None else br.grad}


def gelu_linear_abs(h, w, b, res, gy, add, config="int"):
    """In quanta: GELU(h) counts in units of 16, a hi + lo weight in units of 2^-9."""
    a = hard_gelu(h)[0] / GELU_Q
    qw = E.LO_Q if config == "w_hilo" else 1.0
    aw, ag = w.double().abs() / qw, gy.double().abs()
    y = a @ aw.t() + (0 if b is None else b.double().abs() / (GELU_Q * qw)) + (0 if res is None else res.double().abs() / (GELU_Q * qw))
    dx = (ag @ aw) + (0 if add is None else add.double().abs() / qw)
    return {"y": y.max().item(), "dx": dx.max().item() * 2, "dw": (ag.t() @ a).max().item(), "db": ag.sum(0).max().item()}


def gelu_contrib(h):
    """`contrib` of thin_rows for the GELU Linear: GELU(h) / 16 of the token (dW) and one (dbias)."""
    a = torch.cat([hard_gelu(h)[0] / GELU_Q, torch.ones(h.shape[0], 1, dtype=torch.float64)], 1)
    return lambda idx: a[idx]


def ones_contrib(n_rows):
    """`contrib` of thin_rows behind a LayerNorm: |x-hat| = 1 in every channel, and the ones column of dbias."""
    return lambda idx: torch.ones(len(idx), 1, dtype=torch.float64)


# ---------------------------------------------------------------------------------------------------------------------
# the fused Mlp: Y = X + fc2(GELU(fc1(LayerNorm(X))))
# ---------------------------------------------------------------------------------------------------------------------
def mlp_operands(M, C, hid, mode, seed):
    """{"rows", "gamma", "beta", "w1", "b1", "w2", "b2", "dy"}: W1 = 16 t / gamma, t in {-1, 0, 1} with 2 .. 4 nonzero entries per
    hidden unit (the folded W1 gamma = 16 t is bf16-exact, |h| stays small and max(h, 0) is bf16-representable); b1 is chosen so
    that b1' = b1 + W1 beta is 0 where the unit has an even number of entries and +-16 where it is odd (every unit then reaches
    all three classes); W2 in {-1, 0, 1} with 2 .. 4 nonzero entries per hidden unit, b2 small integers, dY dense integers in
    [-2, 2]."""
    rows = ln_rows(M, C, mode, seed)
    gamma, beta = ln_affine(C, seed + 1)
    t = sparse_ints((hid, C), seed + 2, nnz=(2, 3, 4, 2, 4))
    w1 = t * GELU_Q / gamma
    g = E._rng(seed + 3)
    odd = (t != 0).sum(1) % 2
    b1p = GELU_Q * odd.double() * torch.from_numpy(2 * g.integers(0, 2, size=hid) - 1).double()
    b1 = (b1p - w1.double() @ beta.double()).float()
    w2 = sparse_ints((hid, C), seed + 4, nnz=(2, 4, 3)).t().contiguous()
    return {"rows": rows, "gamma": gamma, "beta": beta, "w1": w1, "b1": b1, "w2": w2, "b2": E.ints((C,), seed + 5, -3, 3),
            "dy": E.ints((M, C), seed + 6, -2, 2)}


def mlp_h(op):
    """The hard pre-activation (M, hid), float64."""
    z = op["gamma"].double() * op["rows"]["sigma"] + op["beta"].double()
    return z @ op["w1"].double().t() + op["b1"].double()


def mlp_hard(op, gy=None):
    """{"y", "dw1", "db1", "dw2", "db2", "dlw", "dlb"} exact; "g" the input of `ln_dx` (the residual dY is its addend)."""
    rows = op["rows"]
    sigma = rows["sigma"]
    z = op["gamma"].double() * sigma + op["beta"].double()
    h = mlp_h(op)
    a, d = hard_gelu(h)
    out = {"h": h, "y": rows["x"].double() + a @ op["w2"].double().t() + op["b2"].double()}
    if gy is not None:
        G = gy.double()
        u = d * (G @ op["w2"].double())                       # dH' (M, hid)
        dz = u @ op["w1"].double()
        out.update({"dw2": G.t() @ a, "db2": G.sum(0), "dw1": u.t() @ z, "db1": u.sum(0), "dlw": (dz * sigma).sum(0), "dlb": dz.sum(0),
                    "g": dz * op["gamma"].double(), "u": u, "G1": u.t() @ sigma})
    return out


def mlp_true(op, gy, eps=LN_EPS):
    """The definition: float64 autograd, LayerNorm with eps (or 0), erf GELU."""
    names = ("gamma", "beta", "w1", "b1", "w2", "b2")
    xr = op["rows"]["x"].double().clone().requires_grad_(True)
    p = {k: op[k].double().clone().requires_grad_(True) for k in names}
    h = F.linear(F.layer_norm(xr, (xr.shape[-1],), p["gamma"], p["beta"], eps), p["w1"], p["b1"])
    y = xr + F.linear(gelu64(h), p["w2"], p["b2"])
    y.backward(gy.double())
    return {"y": y.detach(), "dx": xr.grad, "dw1": p["w1"].grad, "db1": p["b1"].grad, "dw2": p["w2"].grad, "db2": p["b2"].grad,
            "dlw": p["gamma"].grad, "dlb": p["beta"].grad}


def mlp_abs(op, gy):
    """The absolute sums of R2 / R3 per output (maxima).  G1 (= dH'^T x-hat, quantum 1/2) and dW2 (quantum 16) pass through
    bf16 partial sums in rdst_mlp_bwd: they are given in quanta."""
    sigma = op["rows"]["sigma"]
    az = op["gamma"].double() * sigma.abs() + op["beta"].double().abs()
    a, d = hard_gelu(mlp_h(op))
    ag, aw1, aw2 = gy.double().abs(), op["w1"].double().abs(), op["w2"].double().abs()
    u = d * (ag @ aw2)
    dz = u @ aw1
    return {"y": (op["rows"]["x"].double().abs() + a @ aw2.t() + op["b2"].double().abs()).max().item(),
            "h": (az @ aw1.t() + op["b1"].double().abs()).max().item(),
            "dw2": (ag.t() @ (a / GELU_Q)).max().item(), "db2": ag.sum(0).max().item(), "G1": 2 * u.sum(0).max().item(),
            "db1": 2 * u.sum(0).max().item(), "dw1": (u.t() @ az).max().item(), "dlw": dz.sum(0).max().item(), "dlb": dz.sum(0).max().item(),
            "u": u.max().item()}


def mlp_contrib(op):
    """`contrib` of thin_rows for rdst_mlp_bwd: one unit of |dY| in every channel of a token adds GELU(h) / 16 to the column of
    dW2, one to db2, and 2 GELU'(h) sum_c |W2[c, j]| to G1 and db1 (quantum 1/2)."""
    a, d = hard_gelu(mlp_h(op))
    c = torch.cat([a / GELU_Q, 2 * d * op["w2"].double().abs().sum(0), torch.ones(a.shape[0], 1, dtype=torch.float64)], 1)
    return lambda idx: c[idx]


def mlp_thin_gy(op, seed):
    M, C = op["rows"]["x"].shape
    return E.thin_rows(M, M, C, seed, mlp_contrib(op), E.LIMIT_BF16)


# ---------------------------------------------------------------------------------------------------------------------
# the cases of test_exact_ln_gpu.py (test_exact_ln_host.py checks every one of them on the CPU)
# ---------------------------------------------------------------------------------------------------------------------
MODES = E.MODES
LN_CONFIG = {"f32": "int", "bf16": "int", "f32x3": "w_hilo"}      # fp32x3: the hi + lo operand is the weight
# (M, K, N): norm1 + qkv, norm2 + fc1, and one off-size shape ...
LN_LINEAR_SHAPES = [(256, 60, 180), (200, 90, 270), (288, 120, 360), (256, 60, 120), (165, 90, 180), (160, 120, 240), (77, 62, 100)]
# ... and the same widths with enough tokens for the one-pass backward kernels: they keep G (N, K + 1) in the M K floats of the
# dA scratch (lin_bwd_layout, linear.h:40-42), so a call with N (K + 1) > M K goes to the composed backward whatever its scale -
# five of the seven shapes above do.  Ragged M: the last 32-token tile is partial.
LN_LINEAR_SHAPES += [(229, 60, 120), (301, 90, 270), (397, 120, 360), (205, 90, 180), (275, 120, 240), (133, 62, 100)]
# (M, K = hid, N = C): GELU + fc2 + residual
GELU_LINEAR_SHAPES = [(200, 120, 60), (165, 180, 90), (160, 240, 120), (77, 100, 62)]
MLP_FWD_SHAPES = [(7, 60, 120), (165, 60, 120), (293, 90, 180), (288, 120, 240), (77, 62, 100), (64, 124, 232), (65573, 60, 120)]
MLP_BWD_SHAPES = [(7, 60, 120), (165, 60, 120), (293, 90, 180), (288, 120, 240), (77, 62, 100), (64, 124, 232), (16421, 60, 120)]
# fp32 roundings on the longest path of a term of the LayerNorm backward (DESIGN.md section 2 has the kernels and lines): fl(1 / K),
# sum * invK, x-hat * s2, the two subtractions of g - s1 - t, the product with rstd and the rounding of rstd itself are 7 where
# the addend enters through the same fma (the one-pass kernels: mlp_mfma.hip:459, lnlin_mfma.hip:309, lnlin3_mfma.hip:326,
# lnlin3x_mfma.hip:479) and 8 where it is added afterwards (the composed backward: linear_mfma.hip:945-951, :640;
# linear.hip:401-403).  The kernels behind ops.ln_linear take (mean, rstd) from the forward kernel: var * invK, + eps and the
# reciprocal square root are three more (N_FWD_STATS).
# In the fp32 modes a wide Linear (fp32 qkv at C = 90 / 120: N K floats do not fit the LDS) has its data gradient formed as
# LN'(dY[:, :N1] W[:N1]) + LN'(dY[:, N1:] W[N1:]), N1 = ceil4(N / 2), the second launch adding onto the first
# (linear.hip:495-508): one more rounding, and the terms are those of the two halves (`ln_dx_abs_halves`).  Which shapes take
# that route depends on the LDS budget, so the fp32 modes are held to the bound of that route everywhere: 9 roundings on the
# absolute sum over the halves, which is never smaller than the whole's.
N_LN_BWD_ONEPASS, N_LN_BWD, N_LN_BWD_HALVES, N_FWD_STATS = 7, 8, 9, 3


def ln_onepass(mode, sc, M, K, N):
    """Whether rdst_ln_linear_bwd runs the one-pass bf16 kernels (lnlin_mfma.hip, lnlin3_mfma.hip) on this call, read from
    linear.hip:482-487, lnlin_mfma.hip:382 and linear.h:40-42: bf16, everything requested, out_scale 1, K <= 128, and room for G."""
    return mode == "bf16" and sc == 1.0 and K <= 128 and N * (K + 1) <= M * K


def n_ln_bwd(mode, sc, M, K, N):
    """7 in the one-pass bf16 kernels, 8 in the composed bf16 backward, 9 in the fp32 modes (see above)."""
    if mode != "bf16":
        return N_LN_BWD_HALVES
    return N_LN_BWD_ONEPASS if ln_onepass(mode, sc, M, K, N) else N_LN_BWD


@functools.lru_cache(maxsize=None)
def ln_linear_case(M, K, N, mode, seed=4000):
    """Operands of one LayerNorm + Linear case with its dense and thinned dY, the hard results and the absolute sums; computed
    once and read only."""
    config = LN_CONFIG[mode]
    rows = ln_rows(M, K, mode, seed)
    gamma, beta = ln_affine(K, seed + 1)
    w = E.hilo((N, K), seed + 2) if config == "w_hilo" else sparse_ints((N, K), seed + 2, nnz=(K // 4,), hi=2)
    op = {"rows": rows, "gamma": gamma, "beta": beta, "w": w, "b": E.ints((N,), seed + 3, -4, 4), "res": E.ints((M, N), seed + 4, -8, 8),
          "add": E.ints((M, K), seed + 5, -8, 8), "config": config}
    dense = E.dense_gy((M, N), seed + 6)
    draws = [("dense", dense, None)]
    if mode == "bf16":       # G = dY^T x-hat passes through bf16 partial sums: |x-hat| = 1, so at most 256 tokens carry a gradient
        gt, trows = E.thin_rows(M, M, N, seed + 7, ones_contrib(M), E.LIMIT_BF16)
        draws.append(("thin", gt, trows))
        keep = rows["s"] >= 8      # ... and the same with the gradient on rows of s >= 8 only: exact on every route (see `unnarrowed`)
        draws.append(("thin8", gt * keep[:, None], trows[keep[trows]]))
    elif config == "w_hilo":  # d(gamma), d(beta) sum |dY| |W| over tokens AND outputs in quanta of 2^-9: R2 allows a few dozen tokens
        tokens = int((E.LIMIT_F32 - 1) * E.LO_Q / w.abs().double().sum(0).max().item())
        gt, trows = E.thin_rows(M, M, N, seed + 7, ones_contrib(M), float(tokens))
        draws.append(("thin", gt, trows))
    op["draws"] = draws
    return op


def ln_linear_asserted(mode, name):
    """Which outputs a draw is compared on: bf16 - y and dX on the dense draw, the parameter gradients on the thinned one (R3)."""
    if mode == "f32":
        return ("y", "dx", "dw", "db", "dlw", "dlb")
    if mode == "f32x3":      # the hi + lo weight: d(gamma) / d(beta) on the thinned draw (R2)
        return ("y", "dx", "dw", "db") if name == "dense" else ("y", "dx", "dw", "db", "dlw", "dlb")
    return ("y", "dx") if name == "dense" else ("y", "dx", "dw", "db", "dlw", "dlb")      # thin: dW, d(gamma) bounded; thin8: exact


@functools.lru_cache(maxsize=None)
def gelu_linear_case(M, K, N, mode, seed=5000):
    config = LN_CONFIG[mode]
    h = hard_h((M, K), seed)
    w = E.hilo((N, K), seed + 1) if config == "w_hilo" else E.ints((N, K), seed + 1, -2, 2)
    op = {"h": h, "w": w, "b": E.ints((N,), seed + 2, -4, 4), "res": E.ints((M, N), seed + 3, -8, 8), "add": E.ints((M, K), seed + 4, -8, 8),
          "config": config}
    dense = E.dense_gy((M, N), seed + 5)
    draws = [("dense", dense, None)]
    if mode == "bf16":
        gt, trows = E.thin_rows(M, M, N, seed + 6, gelu_contrib(h), E.LIMIT_BF16)
        draws.append(("thin", gt, trows))
    op["draws"] = draws
    return op


def gelu_linear_asserted(mode, name):
    if mode != "bf16":
        return ("y", "dx", "dw", "db")
    return ("y", "dx") if name == "dense" else ("y", "dx", "dw", "db")


@functools.lru_cache(maxsize=None)
def mlp_case(M, C, hid, seed=6000):
    """One fused-Mlp case (bf16): operands, the thinned dY, the hard results on both draws."""
    op = mlp_operands(M, C, hid, "bf16", seed)
    gt, trows = mlp_thin_gy(op, seed + 7)
    op["thin"], op["thin_rows"] = gt, trows
    op["hard_dense"] = mlp_hard(op, op["dy"])
    op["hard_thin"] = mlp_hard(op, gt)
    return op


# ---------------------------------------------------------------------------------------------------------------------
# the preconditions of a draw, asserted on the CPU before every launch (and by test_exact_ln_host.py)
# ---------------------------------------------------------------------------------------------------------------------
# out_scale of the Linear cases: 1 is what the Swin blocks pass and the only scale the one-pass backward kernels take
# (lnlin_mfma.hip:382, lnlin3x_mfma.hip:644); 1/2 sends the same call to the composed backward of linear_mfma.hip
SCALES = (1.0, 0.5)


def _hilo_name(config):
    return {"int": None, "w_hilo": "w"}[config]


def check_ln_rules(op, gy, asserted, mode, sc):
    """R1 - R3 and the statistics of one LayerNorm + Linear draw, on the CPU."""
    rows = op["rows"]
    b = ln_linear_abs(rows, op["gamma"], op["beta"], op["w"], op["b"], op["res"], gy)
    q = E.LO_Q if op["config"] == "w_hilo" else 1.0
    bounds = {"y": b["y"] / (0.5 * q), "dx": b["dA"] / q, "dw": b["dw"] / 0.5, "db": b["db"], "dlw": b["dlw"] / q, "dlb": b["dlb"] / q}
    E.check_rules({"x": rows["x"] if mode == "bf16" else None, "gamma": op["gamma"], "beta": op["beta"], "w": op["w"], "b": op["b"],
                   "res": op["res"], "dy": gy}, _hilo_name(op["config"]), sc, bounds, list(asserted), "f32")
    if mode == "bf16" and "dw" in asserted:      # what passes through the bf16 slabs: G = dY^T x-hat and dbias
        assert b["G"] <= E.LIMIT_BF16 and b["db"] <= E.LIMIT_BF16, f"R3: {b['G']}, {b['db']} > 256 behind bf16 partials"
    for route in STAT_ROUTES:
        mean, rstd = emulate_stats(rows["x"], route)
        assert torch.equal(mean.double(), rows["m"]), f"the mean is not exact on the route {route}"
        big = rows["s"] >= 8
        assert torch.equal(rstd.double()[big], 1.0 / rows["s"][big]), f"rstd is not exact on the route {route}"
        assert mode == "bf16" or bool(big.all())


def check_gelu_rules(op, gy, asserted, mode, sc):
    bounds = gelu_linear_abs(op["h"], op["w"], op["b"], op["res"], gy, None, op["config"])
    E.check_rules({"h": op["h"], "w": op["w"], "b": op["b"], "res": op["res"], "dy": gy}, _hilo_name(op["config"]), sc, bounds, asserted, mode)
    assert_classes(op["h"], "GELU Linear")


def check_mlp_rules(op, gy, asserted):
    rows = op["rows"]
    b = mlp_abs(op, gy)
    for k in ("x",):
        assert E.is_bf16(rows[k])
    for k in ("gamma", "beta", "b1", "w2", "b2"):
        assert E.is_bf16(op[k]), f"R1: {k}"
    assert E.is_bf16(op["w1"] * op["gamma"]) and E.is_bf16(gy), "R1: W1 gamma / dY"
    h = mlp_h(op)
    assert_classes(h, "fused Mlp")
    assert E.is_bf16(hard_gelu(h)[0].float()) and b["h"] < E.LIMIT_F32 and b["y"] * 2 < E.LIMIT_F32, "R1 / R2: h, y"
    assert b["u"] * 2 <= E.LIMIT_BF16, "R1: dH' is not bf16-representable"
    for k in asserted:
        assert b[k] < E.LIMIT_F32, f"R2: {k}"
    if "dw2" in asserted:
        for k in ("G1", "db1", "dw2", "db2"):
            assert b[k] <= E.LIMIT_BF16, f"R3: the absolute sum of {k} is {b[k]} quanta > 256 behind bf16 partials"
    for route in STAT_ROUTES:
        mean, rstd = emulate_stats(rows["x"], route)
        assert torch.equal(mean.double(), rows["m"]), f"the mean is not exact on the route {route}"


RSTD_ULPS_SQRT, RSTD_ULPS_RSQ = 4, 6


def rstd_tol(rows, C, route):
    """How far the rstd a forward kernel writes may be from the float64 one, per row (DESIGN.md has the count).  The argument
    sq * fl(1 / C) + eps carries the rounding of fl(1 / C), of the product or its contraction, and of the sum (2^-24 each, halved
    by the square root: 1.5 ulps of 2^-24); `1.0f / sqrtf` adds a correctly rounded square root and division (one each: 4 in
    all, RSTD_ULPS_SQRT), the reciprocal square root of the streaming kernels is good to 2 ulps of 2^-23 (6 in all,
    RSTD_ULPS_RSQ).  mlp_mfma.hip's forward combines per-chunk (sum, M2) pairs: where the row's last chunk has a length that
    is no power of two (C = 62: 6) its mean sum * fl(1 / 6) is rounded, which moves M2 by 12 d (mu - mean), d <= 2^-23 (|m| + s)."""
    rstd = true_rstd(rows["s"])
    ulps = torch.full_like(rstd, float(RSTD_ULPS_RSQ if route != "null" else RSTD_ULPS_SQRT))
    nlast = C - 8 * ((C + 7) // 8 - 1)
    if route == "null" and (nlast & (nlast - 1)):
        ulps = ulps + (2 * nlast / C) * (rows["m"].abs() / rows["s"] + 1.0)
    return ulps * U24 * rstd


def chunks_exact(C):
    """mlp_mfma.hip's forward sums a row in 16-byte chunks (8 elements, the last C - 8 (ceil(C / 8) - 1)): with a power-of-two
    last chunk every chunk mean and M2 is exact on hard rows, and the kernel's rstd is the contracted formula's."""
    nlast = C - 8 * ((C + 7) // 8 - 1)
    return (nlast & (nlast - 1)) == 0


def rstd_rel(rows):
    """The relative distance of a forward kernel's rstd from 1 / s: eps / (2 s^2) (5e-6 at s = 1) and RSTD_ULPS_RSQ ulps."""
    return LN_EPS / (2 * rows["s"] ** 2) + RSTD_ULPS_RSQ * U24


def mlp_y_tol(op, ref):
    """What the forwards that do not form x-hat may miss y by, beyond its one rounding to bf16.  They evaluate
    h = fma(rstd, acc, fma(-rstd mean, S, b1')) on the raw rows with an rstd that is (1 + e) / s, e = rstd_rel: the factor
    reaches h - b1' as a whole, and the three roundings of the fma chain (and that of -rstd mean) reach the raw sums,
    A_h = (|acc| + |mean S|) / s + |b1'|.  At |h| >= 16 this is far below the bf16 rounding of h GELU; at h = 0 it leaves
    GELU(dh), at most |dh|, in place of 0, which reaches y through |W2|."""
    rows = op["rows"]
    w1g = (op["w1"] * op["gamma"]).double()
    b1p = op["b1"].double() + op["w1"].double() @ op["beta"].double()
    acc = rows["x"].double().abs() @ w1g.abs().t()
    Ah = (acc + rows["m"].abs()[:, None] * w1g.sum(1).abs()[None]) / rows["s"][:, None] + b1p.abs()
    dh = roundings(4) * Ah + rstd_rel(rows)[:, None] * (ref["h"] - b1p).abs()
    return (dh * (ref["h"] == 0)) @ op["w2"].double().abs().t()


def ln_y_tol(op, sc):
    """The same for y of ops.ln_linear in bf16 (lin3_mfma.hip works on the raw rows): sc (e |y - b'| + ((1 + 2^-24)^4 - 1) A),
    A = (|acc| + |mean S|) / s + |b'| <= (2 |m| / s + 1) sum |W gamma| + |b'|; every y may be an exact zero or a tie."""
    rows = op["rows"]
    wg = (op["w"].double() * op["gamma"].double()).abs()
    bp = (op["b"].double() + op["w"].double() @ op["beta"].double()).abs()
    A = (2 * rows["m"].abs() / rows["s"] + 1.0)[:, None] * wg.sum(1)[None] + bp[None]
    return sc * (rstd_rel(rows)[:, None] * wg.sum(1)[None] + roundings(4) * A)


def unnarrowed(rows):
    """e per row: how far x-hat is from +-1 in a bf16 kernel that does NOT narrow it (the composed backward that bwd_t of
    linear.hip falls to keeps x-hat in fp32: linear_mfma.hip:920, :944): eps / (2 s^2) at s < 8 plus the rounding of rstd and of
    the product; at s >= 8 the forward's rstd is 1 / s and x-hat is +-1 in fp32 too (two roundings are left for dX)."""
    s = rows["s"]
    return torch.where(s < 8, LN_EPS / (2 * s ** 2) + 2 * U24, 2 * U24 * torch.ones_like(s))


def ln_wgrad_tol(op, gy, sc):
    """{"dw", "dlw"} for the composed bf16 backward on a draw with rows of s < 8: sum_t |G| gamma e_t (dW) and sum_t |dA| e_t
    (d(gamma)), plus the roundings of a sum that is no longer one of integers: one per 16-token MFMA step, 8 + 8 in the two levels
    of the slab sum (reduce_batch.hip:59-86) and the fma and the scale of the finish (:116) for dW; d(gamma) adds the finish's chain
    over 128-row strides and its two fixed-order levels of 16 and 8 (:112-137)."""
    rows = op["rows"]
    M, N = rows["x"].shape[0], op["w"].shape[0]
    e = unnarrowed(rows)[:, None]
    G = gy.double().abs() * sc
    az = op["gamma"].double() * rows["sigma"].abs() + op["beta"].double().abs()
    n_dw = (M + 15) // 16 + 18
    n_dlw = n_dw + (N + 127) // 128 + 24
    dA = G @ op["w"].double().abs()
    return {"dw": (G * e).t() @ (op["gamma"].double() * rows["sigma"].abs()) + roundings(n_dw) * (G.t() @ az),
            "dlw": (dA * e).sum(0) + roundings(n_dlw) * dA.sum(0)}
