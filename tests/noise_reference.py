"""The float64 reference of the noise term of the device data path (include/rdst_hip_noise.h), shared by test_noise_host.py and
test_noise_gpu.py: Philox4x32-10 in exact integers, the two uniforms, Box-Muller and the two models.  It shares no code with
rdst_amd: the generator is held by the Random123 known-answer vectors (KAT), the rest is the header's definition restated."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
HETERO, RICIAN = 0, 1
SEED = 0x0123456789ABCDEF          # the seed of the statistics, on the host and on the device
# c0 c1 c2 c3 / k0 k1 -> words (Random123, kat_vectors: philox4x32 10)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Counter words (arrays or ints below 2^32) and key words -> the four output words, uint32 arrays.  uint64 arithmetic: a
    product of two 32-bit values fits, so the high and low halves are exact."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(MASK) for c in (c0, c1, c2, c3))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = int(k0) & MASK, int(k1) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & np.uint64(MASK),
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & np.uint64(MASK))
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def words(planes, H, W, seed, plane0=0):
    """uint32 (planes, H, W, 4): key = the seed's halves, counter = (x, y, plane, 0)."""
    p, y, x = np.meshgrid(np.arange(plane0, plane0 + planes), np.arange(H), np.arange(W), indexing="ij")
    return np.stack(philox4x32_10(x, y, p, 0, seed & MASK, (seed >> 32) & MASK), axis=-1)


def normals(w):
    """(z0, z1) float64 from words (..., 4): u1 in (0, 1], u2 in [0, 1)."""
    u1 = ((w[..., 0] >> 8).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (w[..., 1] >> 8).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)


def apply(v, w, model, p0, p1, clip=None):
    """The noisy value and the local noise scale, float64: v (N, C, H, W), w its words (N * C, H, W, 4) reshaped here, p0 / p1
    (N,) levels of the images (taken as the fp32 values the device reads)."""
    v = np.asarray(v, dtype=np.float64)
    z0, z1 = (z.reshape(v.shape) for z in normals(w))
    p0 = np.maximum(np.asarray(p0, dtype=np.float64), 0.0).reshape(-1, 1, 1, 1)
    p1 = np.maximum(np.asarray(p1, dtype=np.float64), 0.0).reshape(-1, 1, 1, 1)
    if model == RICIAN:
        scale = np.broadcast_to(p0, v.shape)
        y = np.hypot(v + p0 * z0, p0 * z1)
    else:
        scale = np.sqrt(p0 * np.maximum(v, 0.0) + p1 * p1)
        y = v + scale * z0
    if clip is not None:
        y = np.clip(y, clip[0], clip[1])
    return y, scale


def ulp32(x):
    """The spacing of fp32 at |x| (of the value rounded to fp32), float64."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def corr(a, b):
    a, b = np.ravel(a) - np.mean(a), np.ravel(b) - np.mean(b)
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def field_stats(z0, z1):
    """What both statistics tests hold of a field of normals (planes, H, W): means, variances, the correlation of the two
    components and the lag-1 correlations of z0 along x and y."""
    return {"mean0": float(z0.mean()), "mean1": float(z1.mean()), "var0": float(z0.var()), "var1": float(z1.var()),
            "corr01": corr(z0, z1), "lag_x": corr(z0[..., :, :-1], z0[..., :, 1:]), "lag_y": corr(z0[..., :-1, :], z0[..., 1:, :])}
