"""Shared helpers for the test-suite."""
import os

import numpy as np
import torch

from oracle import rdst_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

NET_CASES = {
    "net_tiny_64": (O.CFG_TINY, 1),
    "net_tiny_b4": (O.CFG_TINY, 1),      # BASELINE.json configs[0] at its stated shape 4 x 1 x 64 x 64, all gradients elementwise
    "net_e1_16": (O.CFG_E1, 2),
    "net_e1_eval_40x32": (O.CFG_E1, 2),
    "net_ws16_32": (O.make_cfg(**{**O.CFG_WS16, "img_size": 32, "dense_layer_depths": [2, 2], "num_heads": [6, 6],
                                  "window_size": [16, 16], "rdb_depths": [3, 2]}), 3),
    "net_3conv_x3": (O.make_cfg(img_size=16, in_chans=1, sr_scale=3, embed_dim=48, dense_layer_depths=[2],
                                num_heads=[6], window_size=[8], rdb_depths=[2], mlp_ratio=2.0, growth_rate=24,
                                pre_norm=False, resi_connection="3conv", feature_last_operation=False,
                                dense_scale=0.5, rdb_residual_scale=0.7, global_res_scale=0.9), 4),
}


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))


def rand(shape, seed, scale=1.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((scale * rng.standard_normal(shape)).astype(np.float32))


def build_net(cfg, mean=None, std=None, **extra):
    """The HIP-backed RDSTSR for an oracle cfg dict (same kwargs the golden generator gave the reference); `extra`: further
    constructor arguments (drop_rate, attn_drop ...)."""
    import torch.nn as nn
    from rdst_amd.networks.rdst_variations import RDSTSR
    return RDSTSR(
        img_size=cfg["img_size"], patch_size=1, in_chans=cfg["in_chans"], sr_scale=cfg["sr_scale"],
        embed_dim=cfg["embed_dim"], dense_layer_depths=cfg["dense_layer_depths"], num_heads=cfg["num_heads"],
        window_size=cfg["window_size"], rdb_depths=cfg["rdb_depths"], mlp_ratio=cfg["mlp_ratio"],
        qk_scale=cfg["qk_scale"], norm_layer=nn.LayerNorm if cfg["layer_norm"] else nn.Identity,
        patch_norm=cfg["patch_norm"], resi_connection=cfg["resi_connection"], growth_rate=cfg["growth_rate"],
        dense_scale=cfg["dense_scale"], rdb_residual_scale=cfg["rdb_residual_scale"],
        global_res_scale=cfg["global_res_scale"], mean=mean, std=std, pre_norm=cfg["pre_norm"],
        feature_last_operation=cfg["feature_last_operation"], **extra)


def seeded_fill(state_dict, seed):
    """Deterministic weights for ANY module, keyed by state-dict name (numpy PCG64): the golden generator
    fills the reference with it, the tests fill the HIP module with it; integer buffers, masks and MeanShift
    tensors keep their constructed values."""
    import zlib
    out = {}
    for k, v in state_dict.items():
        if (not v.dtype.is_floating_point) or k.endswith("attn_mask") or k.startswith(("sub_mean.", "add_mean.")):
            out[k] = v.clone()
            continue
        rng = np.random.Generator(np.random.PCG64([seed, zlib.crc32(k.encode())]))
        n = torch.from_numpy(rng.standard_normal(tuple(v.shape)).astype(np.float32))
        if k.endswith("relative_position_bias_table"):
            a = 0.5 * n
        elif v.dim() == 1 and k.endswith("weight"):
            a = 1.0 + 0.1 * n            # LayerNorm weight
        elif v.dim() == 1:
            a = 0.05 * n                 # biases
        elif v.dim() == 4:
            a = n / float(np.sqrt(v.shape[1] * v.shape[2] * v.shape[3]))
        elif v.dim() == 2:
            a = 0.7 * n / float(np.sqrt(v.shape[1]))
        else:
            a = 0.02 * n
        out[k] = a
    return out


MODEL_CASES = {
    # name: (kind, ctor kwargs, input shape, seed, train?)
    "swinir_ps_x4": ("swinir", dict(img_size=16, in_chans=1, embed_dim=60, depths=[2, 2], num_heads=[6, 6], window_size=8,
                                    mlp_ratio=2., upscale=4, img_range=1., upsampler="pixelshuffle", drop_path_rate=0.),
                     (2, 1, 16, 16), 21, True),
    "swinir_psd_x2_rgb": ("swinir", dict(img_size=16, in_chans=3, embed_dim=48, depths=[2], num_heads=[6], window_size=8,
                                         mlp_ratio=2., upscale=2, img_range=255., upsampler="pixelshuffledirect",
                                         drop_path_rate=0.1, resi_connection="3conv"),
                          (1, 3, 16, 24), 22, False),
    "swinir_denoise": ("swinir", dict(img_size=16, in_chans=1, embed_dim=48, depths=[2], num_heads=[6], window_size=8,
                                      mlp_ratio=2., upscale=1, img_range=1., upsampler="", drop_path_rate=0.),
                       (1, 1, 16, 16), 23, True),
    "swinir_nearest_x4": ("swinir", dict(img_size=16, in_chans=3, embed_dim=48, depths=[2], num_heads=[6], window_size=8,
                                         mlp_ratio=2., upscale=4, img_range=1., upsampler="nearest+conv", drop_path_rate=0.),
                          (1, 3, 16, 16), 26, True),
    "rdstsr_n_mlp": ("rdstsr_n", dict(img_size=16, in_chans=1, sr_scale=2, embed_dim=48, dense_layer_depths=[2, 2],
                                      num_heads=[6, 6], window_size=[8, 8], rdb_depths=[2, 2], mlp_ratio=2.,
                                      growth_rate=24, pre_norm=True, global_bottleneck=True, global_bottleneck_ratio=1.,
                                      global_bottleneck_mode="mlp", global_res_scale=0.8),
                     (2, 1, 16, 16), 24, True),
    "rdstsr_n_conv": ("rdstsr_n", dict(img_size=16, in_chans=1, sr_scale=2, embed_dim=48, dense_layer_depths=[2, 2],
                                       num_heads=[6, 6], window_size=[8, 8], rdb_depths=[2, 2], mlp_ratio=2.,
                                       growth_rate=24, pre_norm=True, global_bottleneck=True, global_bottleneck_ratio=1.,
                                       global_bottleneck_mode="conv"),
                      (1, 1, 16, 16), 25, True),
    # constructor branches of RDSTSR the factory can select (rdst_variations.py:286-303 'head' mode, :1398-1399 nn.Identity for
    # rdst_layer_norm = False, :1245-1248 / :1330-1331 absolute position embedding; swin_transformer_sr.py:82 qk_scale)
    "rdstsr_head_pre": ("rdstsr", dict(img_size=16, in_chans=1, sr_scale=2, embed_dim=48, dense_layer_depths=[2], num_heads=[6],
                                       window_size=[8], rdb_depths=[2], mlp_ratio=2., growth_rate=24, dim_modify_mode="head",
                                       pre_norm=True, feature_last_operation=True, dense_scale=0.8),
                        (2, 1, 16, 16), 31, True),
    "rdstsr_head_post": ("rdstsr", dict(img_size=16, in_chans=1, sr_scale=2, embed_dim=48, dense_layer_depths=[2], num_heads=[6],
                                        window_size=[8], rdb_depths=[2], mlp_ratio=2., growth_rate=24, dim_modify_mode="head",
                                        pre_norm=False, rdb_residual_scale=0.9),
                         (1, 1, 16, 16), 32, True),
    "rdstsr_identity_norm": ("rdstsr", dict(img_size=16, in_chans=1, sr_scale=2, embed_dim=48, dense_layer_depths=[2], num_heads=[6],
                                            window_size=[8], rdb_depths=[2], mlp_ratio=2., growth_rate=24, pre_norm=True,
                                            norm_layer="identity", feature_last_operation=True),
                             (1, 1, 16, 16), 33, True),
    "rdstsr_ape": ("rdstsr", dict(img_size=16, in_chans=1, sr_scale=2, embed_dim=48, dense_layer_depths=[2], num_heads=[6],
                                  window_size=[8], rdb_depths=[2], mlp_ratio=2., growth_rate=24, pre_norm=True, ape=True,
                                  feature_last_operation=True),
                   (2, 1, 16, 16), 34, True),
    "rdstsr_qk_scale": ("rdstsr", dict(img_size=16, in_chans=1, sr_scale=2, embed_dim=48, dense_layer_depths=[2], num_heads=[6],
                                       window_size=[8], rdb_depths=[2], mlp_ratio=2., growth_rate=24, pre_norm=True, qk_scale=0.3,
                                       feature_last_operation=True),
                        (1, 1, 16, 16), 35, True),
}


def model_kwargs(kw):
    """MODEL_CASES keeps plain data; 'identity' / 'layernorm' name the norm_layer class."""
    import torch.nn as nn
    kw = dict(kw)
    if "norm_layer" in kw:
        kw["norm_layer"] = {"identity": nn.Identity, "layernorm": nn.LayerNorm}[kw["norm_layer"]]
    return kw


def local_rel(got, want, tiles):
    """Tile-local relative error: ||got - want|| / ||want|| over each block of a tiling, in float64.

    `tiles` maps a dimension to its block length along that dimension ({0: 32, 1: 32}: 32 x 32 tiles of a matrix;
    {0: 1}: one row per block); a dimension not named is taken whole.  A dimension that is not a multiple of its block
    length is zero-padded, so the ragged last block is measured on its real elements, never dropped.  Returns
    (worst, median, index of the worst block), the index as a tuple of block coordinates in the order of sorted(tiles).
    A single relative L2 over a whole tensor lets one bad tile hide among thousands of good ones; this does not."""
    import torch.nn.functional as F
    want = want.to(dtype=torch.float64)
    err = got.to(device=want.device, dtype=torch.float64) - want
    if err.shape != want.shape:
        raise ValueError(f"local_rel: shapes {tuple(got.shape)} and {tuple(want.shape)} differ")
    blk = {d % want.dim(): int(b) for d, b in tiles.items()}
    pad = []
    for d in reversed(range(want.dim())):
        b = blk.get(d)
        pad += [0, (-want.shape[d]) % b if b else 0]
    if any(pad):
        err, want = F.pad(err, pad), F.pad(want, pad)
    shape, order, n = [], [], 0
    for d, s in enumerate(want.shape):
        if d in blk:
            shape += [s // blk[d], blk[d]]
            order.append(n)
            n += 2
        else:
            shape.append(s)
            n += 1
    rest = [i for i in range(n) if i not in order]
    perm = order + rest
    e2 = err.reshape(shape).permute(perm).reshape(*[shape[i] for i in order], -1).pow(2).sum(-1)
    w2 = want.reshape(shape).permute(perm).reshape(*[shape[i] for i in order], -1).pow(2).sum(-1)
    rel = (e2.sqrt() / w2.sqrt().clamp_min(1e-300)).flatten()
    i = int(rel.argmax())
    grid = [shape[j] for j in order]
    idx = []
    for g in reversed(grid):
        idx.append(i % g)
        i //= g
    return rel.max().item(), rel.median().item(), tuple(reversed(idx))


# ---------------------------------------------------------------------------------------------------------------------
# Partial gradient requests (test_partial_grads_gpu.py / test_partial_grads_host.py): the request masks, the float64
# reference, the "wide" row layout and the guarded workspace.
# ---------------------------------------------------------------------------------------------------------------------
ACT_NONE, ACT_GELU, ACT_LEAKY02 = 0, 1, 2

# masks over (dX, dW, dbias, dln_w, dln_b) of rdst_ln_linear_bwd behind a LayerNorm
LIN_MASKS_LN = {
    "all": (1, 1, 1, 1, 1),
    "dx": (1, 0, 0, 0, 0),
    "dw+db": (0, 1, 1, 0, 0),
    "dw": (0, 1, 0, 0, 0),
    "db": (0, 0, 1, 0, 0),
    "dx+dw+dlw+dlb": (1, 1, 0, 1, 1),      # a bias-free Linear
    "dx+dlw+dlb": (1, 0, 0, 1, 1),         # frozen Linear
    "dlw+dlb": (0, 0, 0, 1, 1),
    "dx+dw+db": (1, 1, 1, 0, 0),           # frozen LayerNorm
    "dlw": (0, 0, 0, 1, 0),
    "dlb": (0, 0, 0, 0, 1),
    "dx+db": (1, 0, 1, 0, 0),
}
# ... without a LayerNorm (dln_w / dln_b do not exist)
LIN_MASKS_PLAIN = {
    "all": (1, 1, 1, 0, 0),
    "dx": (1, 0, 0, 0, 0),
    "dw+db": (0, 1, 1, 0, 0),
    "dw": (0, 1, 0, 0, 0),
    "db": (0, 0, 1, 0, 0),
    "dx+dw": (1, 1, 0, 0, 0),
    "dx+db": (1, 0, 1, 0, 0),
}
# ... LayerNorm only (Wt == NULL): every non-empty subset of (dX, dln_w, dln_b)
LN_ONLY_MASKS = {
    "+".join(n for n, f in zip(("dx", "dlw", "dlb"), (a, b, c)) if f): (a, 0, 0, b, c)
    for a in (0, 1) for b in (0, 1) for c in (0, 1) if a or b or c
}
# masks over (dX, dW, dbias) of rdst_conv_bwd: all seven non-empty subsets
CONV_MASKS = {
    "+".join(n for n, f in zip(("dx", "dw", "db"), (a, b, c)) if f): (a, b, c)
    for a in (0, 1) for b in (0, 1) for c in (0, 1) if a or b or c
}


def _act64(h, act):
    import torch.nn.functional as F
    if act == ACT_GELU:
        return O.gelu(h)
    if act == ACT_LEAKY02:
        return F.leaky_relu(h, 0.2)
    if act != ACT_NONE:
        raise ValueError(f"activation code {act}")
    return h


def linear_bwd_ref(x, ln_w, ln_b, w, b, gy, act, scale, add=None, dtype=torch.float64):
    """Every gradient of Y = (f(X) @ W^T + b) * scale for the upstream gradient gy, by torch autograd in `dtype`
    (float64: the reference of the GPU tests): f = LayerNorm (ln_w given), the activation `act`, or identity; w None =
    LayerNorm only.  `add` is dX_add: dX = add + f'(...).  Returns {"dx", "dw", "db", "dlw", "dlb"} (None where the
    operand does not exist); the inputs are left unchanged."""
    import torch.nn.functional as F

    def leaf(t):
        return None if t is None else t.detach().to(dtype).clone().requires_grad_(True)
    xr, lw, lb, wr, br = leaf(x), leaf(ln_w), leaf(ln_b), leaf(w), leaf(b)
    h = F.layer_norm(xr, (xr.shape[-1],), lw, lb, 1e-5) if lw is not None else _act64(xr, act)
    if wr is not None:
        h = F.linear(h, wr, br)
    (h * scale).backward(gy.detach().to(dtype))
    dx = xr.grad if add is None else xr.grad + add.detach().to(dtype)

    def grad(t):
        return None if t is None else t.grad
    return {"dx": dx, "dw": grad(wr), "db": grad(br), "dlw": grad(lw), "dlb": grad(lb)}


def conv_bwd_ref(x, w, b, gy, act, scale, r, add=None, dtype=torch.float64):
    """Every gradient of the conv on rows: x (B, H, W, Cin), w (Cout, Cin, k, k), gy in the output geometry
    (B, H r, W r, Cout / r^2) - activation on the input side, zero padding k // 2, * scale, PixelShuffle(r).
    Returns {"dx", "dw", "db"} in `dtype`, dx token-major like x (+ add)."""
    import torch.nn.functional as F
    xr = x.detach().to(dtype).clone().requires_grad_(True)
    wr = w.detach().to(dtype).clone().requires_grad_(True)
    br = b.detach().to(dtype).clone().requires_grad_(True)
    h = F.conv2d(_act64(xr.permute(0, 3, 1, 2), act), wr, br, padding=w.shape[-1] // 2)
    if r > 1:
        h = F.pixel_shuffle(h, r)
    (h.permute(0, 2, 3, 1) * scale).backward(gy.detach().to(dtype))
    dx = xr.grad if add is None else xr.grad + add.detach().to(dtype)
    return {"dx": dx, "dw": wr.grad, "db": br.grad}


def ln_stats(x):
    """The forward's LayerNorm statistics (M, 2) {mean, rstd} in fp32, from float64 on the host."""
    xf = x.detach().double()
    return torch.stack([xf.mean(-1), (xf.var(-1, unbiased=False) + 1e-5).rsqrt()], 1).float().contiguous()


_INT_OF = {2: torch.int16, 4: torch.int32}
WIDE_FILL = {2: 0x4B4D, 4: 0x4B4D4B4D}      # the (finite) bit pattern of every element outside the slice
# (byte offset of the slice, leading dimension in bytes mod 16) per operand slot: every row starts on a 4-byte
# boundary and none on a 16-byte one (offset 8 with rows 0 mod 16: always 8; offset 4 or 12 with rows 8 mod 16: 4, 12, 4 ...)
WIDE_SLOTS = {"x": (8, 0), "dy": (4, 8), "dx": (8, 0), "add": (12, 8)}


class Wide:
    """A (rows, cols) matrix as a column slice of a wider buffer (rows, ld): `view` is the slice (write the operand into
    it, hand `view.data_ptr()` and `ld` to the kernel), `intact()` says whether every element OUTSIDE the slice still
    holds its fill pattern, bit for bit."""

    def __init__(self, rows, cols, dtype, slot, device="cpu"):
        elt = torch.empty((), dtype=dtype).element_size()
        off_b, mod16 = WIDE_SLOTS[slot]
        self.off = off_b // elt
        ld = self.off + cols + 4 // elt
        while (ld * elt) % 16 != mod16:
            ld += 1
        self.ld, self.cols, self.elt = ld, cols, elt
        self.buf = torch.full((rows, ld), WIDE_FILL[elt], dtype=_INT_OF[elt], device=device).view(dtype)
        self.view = self.buf[:, self.off:self.off + cols]
        for r in range(min(rows, 4)):   # the layout the tests ask for
            a = self.off * elt + r * ld * elt
            assert a % 4 == 0 and a % 16 != 0, (slot, cols, dtype)

    def intact(self):
        bits = self.buf.view(_INT_OF[self.elt])
        fill = torch.full_like(bits[:, :1], WIDE_FILL[self.elt])
        left, right = bits[:, :self.off], bits[:, self.off + self.cols:]
        return bool((left == fill).all()) and bool((right == fill).all())


class GuardedWorkspace:
    """`nbytes` of scratch as the middle of a larger allocation: 4096 sentinel bytes on either side (the second starts at
    byte `nbytes` exactly), the scratch itself filled with 0xFF (fp32 NaN: a kernel that reads scratch nobody wrote shows)."""
    GUARD, SENTINEL = 4096, 0xA5

    def __init__(self, nbytes, device="cpu"):
        self.nbytes = int(nbytes)
        self.buf = torch.full((2 * self.GUARD + self.nbytes,), self.SENTINEL, dtype=torch.uint8, device=device)
        self.buf[self.GUARD:self.GUARD + self.nbytes] = 0xFF

    def ptr(self):
        return self.buf.data_ptr() + self.GUARD

    def intact(self):
        lo, hi = self.buf[:self.GUARD], self.buf[self.GUARD + self.nbytes:]
        return bool((lo == self.SENTINEL).all()) and bool((hi == self.SENTINEL).all())
