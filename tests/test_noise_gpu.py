"""GPU: the noise term of the device data path (csrc/noise.hip: rdst_noise_words, rdst_add_noise; csrc/resample.hip:
rdst_sample_patches_noise) behind rdst_amd.data.noise_words, add_noise, make_test_pair(noise=) and DevicePatchSampler(noise=).
The generator's words against the numpy Philox, exactly; add_noise against the float64 reference made from the same words,
under the bound derived below; the sampler's noisy LR patches against add_noise of the resample of its own HR patches, bit for
bit, across band and chunk seams, turns, labels and degradations; levels per patch; the statistics of the DEVICE field under
the thresholds tests/test_noise_host.py holds for the reference; determinism and independence; the test pair; and
DPTrainStep.step_from under the graph.

The bound: |y - y_ref| <= 2^-16 s + 4 ulp(y_ref), s the local noise scale (sd of the hetero model, sigma of the Rician one).
u1, u2 and the argument of sincospi are exact; z carries the errors of logf, sqrtf, sincospif and one product, and with those
functions at no more than 4 ulp |dz| <= 5.77 (3.0e-7 + 4.8e-7) + 3.4e-7, about 4.8e-6 < 2^-17; the Rician model doubles it
through its two components.  The 4 ulp of the library functions is an assumption; what was measured on an MI355X when the
test was written is a worst |error| / bound of 0.17 (Rician), 0.08 (Gaussian) and 0.04 (Poisson-Gaussian)."""
import math

import numpy as np
import pytest
import torch

import noise_reference as R
from rdst_amd import data as D
from test_data_gpu import _net, _stack
from test_noise_host import N_STAT, T_MEAN, T_VAR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
S, H, W = 6, 56, 60
SHAPES = [(12, 4.0), (5, 2.5)]        # (lp, scale): hp = 48, two column bands (8 + 4) and two row chunks (32 + 16); hp = 12
ALL_TURNS = ([0, 1, 2, 3, 4, 5], [2, 3, 4, 5, 6, 7])         # S = 6 patches per batch: two batches cover the eight
KINDS = ("cubic", "cubic+gaussian", "cubic_aa")
SEED2 = 0xA4093822_299F31D0           # both halves non-zero, the top bit set
NOISES = [D.Noise("gaussian", sigma=(0.01, 0.05)), D.Noise("poisson-gaussian", gain=(0.0, 0.02), sigma=0.01, clip=(0.0, 1.0)),
          D.Noise("rician", sigma=(0.01, 0.05))]


def _draws(hp, seed, turns=None):
    g = torch.Generator().manual_seed(seed)
    idx = torch.stack([torch.randperm(S, generator=g), torch.randint(0, H - hp + 1, (S,), generator=g),
                       torch.randint(0, W - hp + 1, (S,), generator=g)], dim=1).to(torch.int32)
    idx[0, 1:] = 0
    idx[1, 1], idx[1, 2] = H - hp, W - hp
    return idx if turns is None else (idx, torch.tensor(turns, dtype=torch.int32))


def _np_words(t):
    return t.cpu().numpy().view(np.uint32)


def test_noise_words_are_the_numpy_philox():
    for planes, h, w, seed in ((3, 7, 9, SEED2), (8, 64, 64, R.SEED), (2, 5, 300, 1), (1, 1, 1, (1 << 64) - 1)):
        got = D.noise_words(planes, h, w, seed)
        assert got.dtype == torch.int32 and got.shape == (planes, h, w, 4) and got.device == DEV
        want = torch.from_numpy(R.words(planes, h, w, seed).view(np.int32))
        assert torch.equal(got.cpu(), want), (planes, h, w, hex(seed))
    # a plane index > 0 under a seed with both halves non-zero, spelled out
    one = R.philox4x32_10(4, 2, 1, 0, SEED2 & 0xffffffff, SEED2 >> 32)
    assert tuple(int(v) for v in _np_words(D.noise_words(3, 7, 9, SEED2))[1, 2, 4]) == tuple(int(v) for v in one)


@pytest.mark.parametrize("noise", NOISES + [D.Noise("gaussian", sigma=0.3, clip=(0.25, 0.75)), D.Noise("rician", sigma=0.2, clip=(0.1, 0.6))],
                         ids=["gaussian", "poisson-gaussian-clip", "rician", "gaussian-clip", "rician-clip"])
def test_add_noise_against_the_float64_reference(noise):
    N, C, h, w = 3, 2, 37, 41
    g = torch.Generator().manual_seed(11)
    x = torch.rand(N, C, h, w, generator=g) * 1.2 - 0.1           # some values below 0: the hetero model's max(v, 0)
    y, seed, levels = D.add_noise(x.to(DEV), noise, seed=SEED2, generator=g, return_draw=True)
    assert seed == SEED2 and levels.shape == (N, 2) and levels.dtype == torch.float32 and not levels.is_cuda
    words = _np_words(D.noise_words(N * C, h, w, seed))
    assert np.array_equal(words, R.words(N * C, h, w, seed))
    lv = levels.double().numpy()
    clip = None if noise.clip is None else tuple(float(np.float32(c)) for c in noise.clip)      # as the kernel receives them
    want, scale = R.apply(x.double().numpy(), words, noise.model, lv[:, 0], lv[:, 1], clip)
    err = np.abs(y.cpu().double().numpy() - want)
    bound = 2.0 ** -16 * scale + 4 * R.ulp32(want)
    print(f"[noise] {noise!r}: worst |gpu - float64| / bound = {(err / bound).max():.3f}, max|err| = {err.max():.3e}, "
          f"max|err| / scale = {(err / np.maximum(scale, 1e-30)).max():.3e}")
    assert (err <= bound).all()
    assert np.abs(y.cpu().double().numpy() - x.double().numpy()).max() > 0.01          # there is noise
    if noise.clip is not None:
        assert y.min().item() == clip[0] and y.max().item() == clip[1]           # both ends are reached, neither is passed
    # (C, H, W) is image 0 of a batch of one
    y3 = D.add_noise(x[0].to(DEV), noise, levels=levels[:1], seed=seed)
    assert y3.shape == (C, h, w) and torch.equal(y3, y[0])
    # levels that are already on the device
    assert torch.equal(D.add_noise(x.to(DEV), noise, levels=levels.to(DEV), seed=seed), y)


@pytest.mark.parametrize("with_labels", [False, True], ids=["nolabels", "labels"])
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("lp,scale", SHAPES, ids=["hp48", "hp12"])
@pytest.mark.parametrize("kind", KINDS)
def test_sampler_is_add_noise_of_the_resample_of_its_own_output(kind, lp, scale, C, with_labels):
    hp = int(lp * scale)
    imgs, labels = _stack(S, C, H, W, seed=8)
    kw = dict(sr_scales=(scale,), labels=labels if with_labels else None, device=DEV, degradation=kind)
    clean = D.DevicePatchSampler(imgs, S, lp, **kw)
    gl = torch.Generator().manual_seed(17)
    for i, noise in enumerate(NOISES):
        s = D.DevicePatchSampler(imgs, S, lp, noise=noise, **kw)
        plain = [D.Draw(scale, hp, _draws(hp, 5))] + [D.Draw(scale, hp, *_draws(hp, 6 + j, t)) for j, t in enumerate(ALL_TURNS)]
        for j, p in enumerate(plain):
            d = p._replace(noise_seed=SEED2 + 1000 * i + j, noise_levels=noise.levels_from(torch.rand(S, 2, generator=gl)))
            ref, b = clean.sample(draw=p), s.sample(draw=d)
            assert set(b) == set(ref) | {"noise", "noise_seed", "noise_levels"}
            assert b["noise"] == noise and b["noise_seed"] == d.noise_seed and torch.equal(b["noise_levels"], d.noise_levels)
            assert torch.equal(b["out"], ref["out"])
            if with_labels:
                assert torch.equal(b["label"], ref["label"])
            lr = D.resample(b["out"], lp, kind)
            assert torch.equal(lr, ref["in"])
            assert torch.equal(b["in"], D.add_noise(lr, noise, levels=d.noise_levels, seed=d.noise_seed))
            assert not torch.equal(b["in"], ref["in"])
            # a draw without the noise fields through the noisy sampler: the clean batch
            c = s.sample(draw=p)
            assert set(c) == set(ref) and torch.equal(c["in"], ref["in"]) and torch.equal(c["out"], ref["out"])


@pytest.mark.parametrize("augment", [False, True])
@pytest.mark.parametrize("kind", [None, "cubic+gaussian"])
def test_the_free_running_sampler(kind, augment):
    """draw() itself: the same origins and variants as the clean sampler under the same generator seed, the identity for the
    batch it leads to, and noise=None is the sampler built without the argument: the same keys and the same bits."""
    lp, scale = 12, 4.0
    imgs, labels = _stack(S, 2, H, W, seed=9)
    kw = dict(sr_scales=(scale,), labels=labels, device=DEV, augment=augment)
    if kind is not None:
        kw["degradation"] = kind
    g = lambda: torch.Generator().manual_seed(4)
    before = D.DevicePatchSampler(imgs, S, lp, generator=g(), **kw)
    none = D.DevicePatchSampler(imgs, S, lp, generator=g(), noise=None, **kw)
    noise = D.Noise("rician", sigma=(0.0, 0.05), clip=(0.0, 1.0))
    s = D.DevicePatchSampler(imgs, S, lp, generator=g(), noise=noise, **kw)
    seeds = []
    for _ in range(2):
        a, n = before.sample(), none.sample()
        assert set(a) == set(n) and "noise" not in n
        for k in a:
            assert torch.equal(a[k], n[k]) if isinstance(a[k], torch.Tensor) else a[k] == n[k]
        # the noisy sampler has drawn a seed and levels in between, so only its first batch has the clean one's origins
        b = s.sample()
        if not seeds:
            assert torch.equal(b["indices"], a["indices"]) and torch.equal(b["out"], a["out"]) and torch.equal(b["label"], a["label"])
            assert ("variants" in b) == augment and (not augment or torch.equal(b["variants"], a["variants"]))
        lr = D.resample(b["out"], lp, kind or "cubic")
        assert torch.equal(b["in"], D.add_noise(lr, noise, levels=b["noise_levels"], seed=b["noise_seed"]))
        assert b["noise_levels"].shape == (S, 2) and (b["noise_levels"][:, 1] == 0).all() and b["noise_levels"][:, 0].max() <= 0.05
        seeds.append(b["noise_seed"])
    assert seeds[0] != seeds[1]


@pytest.mark.parametrize("kind", KINDS)
def test_levels(kind):
    lp, scale, hp = 12, 4.0, 48
    imgs, _ = _stack(S, 2, H, W, seed=10)
    p = D.Draw(scale, hp, *_draws(hp, 3, ALL_TURNS[1]))
    zeros = torch.zeros(S, 2)
    het = D.DevicePatchSampler(imgs, S, lp, sr_scales=(scale,), device=DEV, degradation=kind, noise="poisson-gaussian")
    b = het.sample(draw=p._replace(noise_seed=5, noise_levels=zeros))
    clean = D.resample(b["out"], lp, kind)
    assert torch.equal(b["in"], clean)                                         # zero levels: the clean path, bit for bit
    ric = D.DevicePatchSampler(imgs - 0.3, S, lp, sr_scales=(scale,), device=DEV, degradation=kind, noise="rician")
    b = ric.sample(draw=p._replace(noise_seed=5, noise_levels=zeros))
    want = D.resample(b["out"], lp, kind).abs()
    assert (b["out"] < 0).any() and ((b["in"] - want).abs().cpu().double().numpy() <= R.ulp32(want.cpu().numpy())).all()
    # per patch: the first half at level 0, the second at 0.05
    half = torch.tensor([[0.0, 0.0]] * 3 + [[0.0, 0.05]] * 3)
    b = het.sample(draw=p._replace(noise_seed=6, noise_levels=half))
    clean = D.resample(b["out"], lp, kind)
    assert torch.equal(b["in"][:3], clean[:3])
    for i in range(3, S):
        d = (b["in"][i] - clean[i]).double()
        assert not torch.equal(b["in"][i], clean[i]) and 0.03 < d.std().item() < 0.07
    half = torch.tensor([[0.0, 0.0]] * 3 + [[0.05, 0.0]] * 3)
    b = ric.sample(draw=p._replace(noise_seed=6, noise_levels=half))
    want = D.resample(b["out"], lp, kind)
    assert ((b["in"][:3] - want[:3].abs()).abs().cpu().double().numpy() <= R.ulp32(want[:3].cpu().numpy())).all()
    assert all((b["in"][i] - want[i].abs()).abs().max().item() > 0.01 for i in range(3, S))


def test_statistics_of_the_device_field():
    """A constant image 0.5 of 8 x 1 x 64 x 64 under seed 0x0123456789ABCDEF: the thresholds of tests/test_noise_host.py."""
    sigma = 0.05
    x = torch.full((8, 1, 64, 64), 0.5, device=DEV)
    lv = torch.tensor([[0.0, sigma]] * 8)
    y = D.add_noise(x, "gaussian", levels=lv, seed=R.SEED)
    z = ((y.cpu().double() - 0.5) / float(np.float32(sigma))).numpy()[:, 0]
    z0_ref, z1_ref = R.normals(R.words(8, 64, 64, R.SEED))
    st = R.field_stats(z, z1_ref)
    print("[device field]", {k: round(v, 5) for k, v in st.items()}, "max|z - z_ref| =", np.abs(z - z0_ref).max())
    assert z.size == N_STAT and abs(st["mean0"]) < T_MEAN and abs(st["var0"] - 1) < T_VAR
    assert abs(st["lag_x"]) < T_MEAN and abs(st["lag_y"]) < T_MEAN and abs(st["corr01"]) < T_MEAN
    # the Rician mean at v = 0: sigma sqrt(pi / 2), within five standard errors
    r = D.add_noise(torch.zeros_like(x), "rician", levels=torch.tensor([[sigma, 0.0]] * 8), seed=R.SEED).cpu().double()
    se = r.std().item() / math.sqrt(r.numel())
    print(f"[device field] Rician mean at 0: {r.mean().item():.6f} against {sigma * math.sqrt(math.pi / 2):.6f}, se {se:.2e}")
    assert abs(r.mean().item() - float(np.float32(sigma)) * math.sqrt(math.pi / 2)) < 5 * se and (r >= 0).all()
    # the hetero model: the variance follows the signal, in the ratio of sd^2
    gain, floor = 0.01, 0.02
    var = {}
    for v in (0.25, 0.75):
        h = D.add_noise(torch.full_like(x, v), "poisson-gaussian", levels=torch.tensor([[gain, floor]] * 8), seed=R.SEED)
        var[v] = (h.cpu().double() - v).var(unbiased=False).item()
        sd2 = float(np.float32(gain)) * v + float(np.float32(floor)) ** 2
        print(f"[device field] hetero v = {v}: var = {var[v]:.6e} against sd^2 = {sd2:.6e}")
        assert abs(var[v] / sd2 - 1) < T_VAR
    assert var[0.75] > 2 * var[0.25]


def test_determinism_and_independence():
    x = torch.rand(8, 1, 64, 64, generator=torch.Generator().manual_seed(2)).to(DEV)
    lv = torch.tensor([[0.0, 0.05]] * 8)
    a, b = D.add_noise(x, "gaussian", levels=lv, seed=R.SEED), D.add_noise(x, "gaussian", levels=lv, seed=R.SEED)
    assert torch.equal(a, b)
    c = D.add_noise(x, "gaussian", levels=lv, seed=R.SEED + 1)
    na, nc = (a - x).cpu().double().numpy(), (c - x).cpu().double().numpy()
    print(f"[independence] two seeds: corr = {R.corr(na, nc):.5f}; two planes: corr = {R.corr(na[:4], na[4:]):.5f}")
    assert abs(R.corr(na, nc)) < T_MEAN
    assert abs(R.corr(na[:4], na[4:])) < 5 / math.sqrt(na[:4].size)
    # in place equals out of place
    for noise in ("gaussian", D.Noise("rician", sigma=0.1, clip=(0.0, 0.9))):
        want = D.add_noise(x, noise, levels=lv, seed=7)
        t = x.clone()
        got = D.add_noise(t, noise, levels=lv, seed=7, out=t)
        assert got is t and torch.equal(t, want) and not torch.equal(t, x)
    # what is drawn is returned, and reproduces the call
    g = torch.Generator().manual_seed(3)
    noise = D.Noise("poisson-gaussian", gain=(0.0, 0.02), sigma=(0.0, 0.03))
    y, seed, levels = D.add_noise(x, noise, generator=g, return_draw=True)
    seed2, levels2 = noise.draw(8, torch.Generator().manual_seed(3))
    assert seed == seed2 and torch.equal(levels, levels2)
    assert torch.equal(D.add_noise(x, noise, levels=levels, seed=seed), y)


def test_add_noise_does_not_wait_for_the_device():
    x = torch.rand(2, 1, 32, 32).to(DEV)
    D.add_noise(x, "gaussian", seed=1)          # the library is loaded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        D.add_noise(x, D.Noise("rician", sigma=(0.0, 0.1)), generator=torch.Generator().manual_seed(1))
        D.add_noise(x, "gaussian", levels=torch.tensor([[0.0, 0.1]] * 2), seed=5, out=x)
    finally:
        torch.cuda.set_sync_debug_mode("default")


@pytest.mark.parametrize("kind", [None, "cubic_aa"])
def test_make_test_pair_with_noise(kind):
    hr = torch.rand(2, 1, 44, 40, generator=torch.Generator().manual_seed(4)).to(DEV)
    noise = D.Noise("rician", sigma=(0.01, 0.05))
    for s in (4, 3):        # gt is hr itself, and gt is a resize of it
        lr0, gt0, rs0 = D.make_test_pair(hr, s, kind)
        keep = hr.clone()
        lr, gt, rs = D.make_test_pair(hr, s, kind, noise=noise, generator=torch.Generator().manual_seed(6), seed=SEED2)
        levels = noise.levels_from(torch.rand(2, 2, generator=torch.Generator().manual_seed(6)))
        assert torch.equal(hr, keep) and torch.equal(gt, gt0) and (gt is hr) == (gt0 is hr) and rs == rs0
        assert torch.equal(lr, D.add_noise(lr0, noise, levels=levels, seed=SEED2)) and not torch.equal(lr, lr0)
        # the seed drawn too: first the seed, then the levels
        lr2, _, _ = D.make_test_pair(hr, s, kind, noise=noise, generator=torch.Generator().manual_seed(6))
        seed, levels = noise.draw(2, torch.Generator().manual_seed(6))
        assert torch.equal(lr2, D.add_noise(lr0, noise, levels=levels, seed=seed))


def test_step_from_with_a_noisy_sampler_under_the_graph():
    """step_from(sampler) with noise on the tiny network of tests/test_data_gpu.py: eager steps, the capture, then replays that
    sample straight into the graph's tensors.  Every batch is add_noise of the resample of its own target under its own seed,
    the seeds differ from step to step, and the losses are finite."""
    from rdst_amd.trainer import DPTrainStep
    imgs, _ = _stack(5, 1, 80, 72, seed=9)
    net = _net("bf16")
    tr = DPTrainStep(net, lr=1e-3, graph=True, graph_warmup=2)
    noise = D.Noise("gaussian", sigma=(0.01, 0.05), clip=(0.0, 1.0))
    s = D.DevicePatchSampler(imgs, 2, 16, sr_scales=(4.0,), device=DEV, generator=torch.Generator().manual_seed(21),
                             degradation="cubic+gaussian", noise=noise)
    losses, seeds, in_place = [], [], []
    for i in range(5):
        losses.append(tr.step_from(s).clone())
        b = tr.last_batch
        assert b["noise"] == noise and b["in"].shape == (2, 1, 16, 16)
        lr = D.resample(b["out"], 16, "cubic+gaussian")
        assert torch.equal(b["in"], D.add_noise(lr, noise, levels=b["noise_levels"], seed=b["noise_seed"]))
        assert not torch.equal(b["in"], lr)
        seeds.append(b["noise_seed"])
        in_place.append(tr._static is not None and b["in"].data_ptr() == tr._static[0].data_ptr()
                        and b["out"].data_ptr() == tr._static[1].data_ptr())
    torch.cuda.synchronize()
    assert tr.graph is not None and in_place == [False] * 3 + [True] * 2
    assert len(set(seeds)) == len(seeds)
    assert all(math.isfinite(l.item()) for l in losses)
