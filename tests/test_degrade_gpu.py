"""GPU: the K-tap degradations (csrc/resample.hip: rdst_resample_sep, rdst_sample_patches_op) behind rdst_amd.data.resample,
make_test_pair(degradation=) and DevicePatchSampler(degradation=).  A 'cubic' table through the new entry points against the
4-tap ones, bit for bit; the sampler's LR patches against the whole-image resample of its HR patches, bit for bit, for every
kind and turn; exact results where the weights are dyadic; the derived fp32 bound against the float64 operator everywhere
else; the test pair; and DPTrainStep.step_from under the graph.  The tables themselves are held in tests/test_degrade_host.py."""
import numpy as np
import pytest
import torch

from rdst_amd import data as D
from test_data_gpu import _net, _stack
from test_degrade_host import NEW_KINDS, bound, dense

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
S, H, W = 6, 40, 44
SHAPES = [(4, 4.0), (5, 2.5), (8, 3.0), (8, 2.0)]          # (lp, scale): hp = 16, 12, 24, 16
ALL_TURNS = ([0, 1, 2, 3, 4, 5], [2, 3, 4, 5, 6, 7])         # S = 6 patches per batch: two batches cover the eight


def _draws(hp, seed, turns=None):
    g = torch.Generator().manual_seed(seed)
    idx = torch.stack([torch.randperm(S, generator=g), torch.randint(0, H - hp + 1, (S,), generator=g),
                       torch.randint(0, W - hp + 1, (S,), generator=g)], dim=1).to(torch.int32)
    idx[0, 1:] = 0
    idx[1, 1], idx[1, 2] = H - hp, W - hp
    return idx if turns is None else (idx, torch.tensor(turns, dtype=torch.int32))


def _float64(kind, x, oh, ow):
    """The float64 operator on a host tensor (N, C, H, W) -> numpy (N, C, oh, ow)."""
    My, Mx = dense(kind, x.shape[-2], oh), dense(kind, x.shape[-1], ow)
    return np.einsum("oh,nchw,pw->ncop", My, x.double().numpy(), Mx)


@pytest.mark.parametrize("shape,size", [((2, 3, 40, 44), (10, 11)), ((1, 1, 15, 22), (6, 5)), ((2, 1, 12, 9), (30, 31)),
                                        ((1, 2, 64, 64), 16)])
def test_cubic_table_through_resample_sep_is_the_bicubic_resize(shape, size):
    x = torch.rand(shape, generator=torch.Generator().manual_seed(1)).to(DEV)
    assert torch.equal(D.resample(x, size, "cubic"), D.bicubic_resize(x, size))
    assert torch.equal(D.resample(x[0], size), D.bicubic_resize(x[0], size))


@pytest.mark.parametrize("with_labels", [False, True], ids=["nolabels", "labels"])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("lp,scale", SHAPES)
def test_cubic_table_through_sample_patches_op_is_the_sampler(lp, scale, C, with_labels):
    """rdst_sample_patches_op under the K = 4 table of tap_table against rdst_sample_patches and rdst_sample_patches_d8: the
    second sampler is the first with its entry point switched (a 'cubic' Degradation normally selects the 4-tap ones)."""
    hp = int(lp * scale)
    imgs, labels = _stack(S, C, H, W, seed=3)
    kw = dict(sr_scales=(scale,), labels=labels if with_labels else None, device=DEV)
    old, new = D.DevicePatchSampler(imgs, S, lp, **kw), D.DevicePatchSampler(imgs, S, lp, **kw)
    new.degradation = D.Degradation("cubic")
    draws = [D.Draw(scale, hp, _draws(hp, 5))] + [D.Draw(scale, hp, *_draws(hp, 6 + i, t)) for i, t in enumerate(ALL_TURNS)]
    for d in draws:
        a, b = old.sample(draw=d), new.sample(draw=d)
        assert set(b) == set(a) | {"degradation"}
        assert torch.equal(a["in"], b["in"]) and torch.equal(a["out"], b["out"])
        if with_labels:
            assert torch.equal(a["label"], b["label"])


@pytest.mark.parametrize("lp,scale", [(4, 4.0), (5, 4.0), (8, 3.0), (6, 2.5)], ids=["hp16", "hp20", "hp24", "hp15"])
@pytest.mark.parametrize("kind", NEW_KINDS)
def test_sampler_is_the_resample_of_its_own_output(kind, lp, scale):
    hp = int(lp * scale)
    imgs, labels = _stack(S, 2, H, W, seed=8)
    kw = dict(sr_scales=(scale,), labels=labels, device=DEV)
    cubic, s = D.DevicePatchSampler(imgs, S, lp, **kw), D.DevicePatchSampler(imgs, S, lp, degradation=kind, **kw)
    draws = [D.Draw(scale, hp, _draws(hp, 5))] + [D.Draw(scale, hp, *_draws(hp, 6 + i, t)) for i, t in enumerate(ALL_TURNS)]
    for d in draws:
        ref, b = cubic.sample(draw=d), s.sample(draw=d)
        assert b["degradation"] == D.Degradation(kind) and ("variants" in b) == (d.variants is not None)
        assert torch.equal(b["out"], ref["out"]) and torch.equal(b["label"], ref["label"])
        assert torch.equal(b["in"], D.resample(b["out"], lp, kind))
        assert not torch.equal(b["in"], ref["in"])
    # the free-running sampler with augment=True: the same generator use as the cubic one, the same identity
    g = lambda: torch.Generator().manual_seed(4)
    a8 = D.DevicePatchSampler(imgs, S, lp, augment=True, generator=g(), **kw)
    s8 = D.DevicePatchSampler(imgs, S, lp, augment=True, generator=g(), degradation=kind, **kw)
    for _ in range(2):
        ref, b = a8.sample(), s8.sample()
        assert torch.equal(b["indices"], ref["indices"]) and torch.equal(b["variants"], ref["variants"])
        assert torch.equal(b["out"], ref["out"]) and torch.equal(b["label"], ref["label"])
        assert torch.equal(b["in"], D.resample(b["out"], lp, kind))


def test_exact_results_with_dyadic_weights():
    """Integer pixels and dyadic weights: every product and partial sum is a multiple of a power of two and fits 24 bits, so
    fp32 must give the float64 result itself.  'cubic+gaussian' at ratio 4 (weights k / 128, sum |w| = 1.375): pixels 0..255,
    horizontal sums multiples of 2^-7 below 512, vertical sums multiples of 2^-14 below 512: 23 bits.  'cubic_aa' at 16 -> 8
    (tests/test_degrade_host.py: dyadic, k / 256, on the output rows and columns 2..5 only; no other size does better): the
    vertical sums are multiples of 2^-16, exact while they stay below 256, which pixels 0..127 and sum |w| < 1.41 ensure."""
    g = torch.Generator().manual_seed(12)
    imgs = torch.randint(0, 256, (S, 1, H, W), generator=g).float()
    assert np.abs(D.operator_table("cubic+gaussian", 16, 4)[1]).sum(1).max() == 1.375
    x = imgs[:, :, :40, :44]
    y = D.resample(x.to(DEV), (10, 11), "cubic+gaussian")
    assert torch.equal(y.cpu().double(), torch.from_numpy(_float64("cubic+gaussian", x, 10, 11)))
    s = D.DevicePatchSampler(imgs, S, 4, degradation="cubic+gaussian", device=DEV)
    for t in ALL_TURNS:
        b = s.sample(draw=D.Draw(4.0, 16, *_draws(16, 2, t)))
        assert torch.equal(b["in"].cpu().double(), torch.from_numpy(_float64("cubic+gaussian", b["out"].cpu(), 4, 4)))
    imgs = torch.randint(0, 128, (S, 1, H, W), generator=g).float()
    wsum = np.abs(D.operator_table("cubic_aa", 16, 8)[1]).sum(1)[2:6].max()
    assert wsum * wsum * 127 < 256
    s = D.DevicePatchSampler(imgs, S, 8, sr_scales=(2.0,), degradation="cubic_aa", device=DEV)
    for t in ALL_TURNS:
        b = s.sample(draw=D.Draw(2.0, 16, *_draws(16, 3, t)))
        want = torch.from_numpy(_float64("cubic_aa", b["out"].cpu(), 8, 8))
        assert torch.equal(b["in"].cpu().double()[..., 2:6, 2:6], want[..., 2:6, 2:6])
        assert torch.equal(D.resample(b["out"], 8, "cubic_aa"), b["in"])


def _hold_bound(kind, got, x, oh, ow, what):
    want = _float64(kind, x, oh, ow)
    b = bound(kind, x.shape[-2], oh, x.shape[-1], ow, float(x.abs().max()))
    ratio = (np.abs(got.cpu().double().numpy() - want) / b).max()
    print(f"[bound] {what} {kind} {tuple(x.shape[-2:])} -> {(oh, ow)}: worst |gpu - float64| / bound = {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("lo", [0.0, 100.0], ids=["unit", "offcentre"])
@pytest.mark.parametrize("kind", D.KINDS)
def test_the_derived_bound_whole_images(kind, lo):
    """|gpu - float64| <= gamma Sy[oy] Sx[ox] max|x| per pixel, gamma = n u / (1 - n u), n = Ky + Kx + 2, u = 2^-24: two chained
    fp32 dot products with once-rounded weights (test_degrade_host.bound; that file holds the gate against mutated operators)."""
    x = lo + torch.rand(2, 2, H, W, generator=torch.Generator().manual_seed(7))
    for oh, ow in ((10, 11), (13, 9), (40, 44)):
        _hold_bound(kind, D.resample(x.to(DEV), (oh, ow), kind), x, oh, ow, "resample")


@pytest.mark.parametrize("lo", [0.0, 100.0], ids=["unit", "offcentre"])
@pytest.mark.parametrize("kind,hp,lp", [(k, 32, 8) for k in NEW_KINDS] + [(k, 24, 5) for k in NEW_KINDS] + [("fourier", 256, 64)])
def test_the_derived_bound_sampler(kind, hp, lp, lo):
    """The sampler's batches; 'fourier' 256 -> 64 with B = 2 is the benchmark's patch, the dense table at its largest."""
    B = 2 if hp == 256 else 4
    imgs = lo + torch.rand(B, 1, hp + 3, hp + 8, generator=torch.Generator().manual_seed(hp))
    s = D.DevicePatchSampler(imgs, B, lp, sr_scales=(hp / lp,), degradation=kind, device=DEV, augment=True,
                             generator=torch.Generator().manual_seed(1))
    assert s.hr_patch_sizes == [hp]
    b = s.sample()
    _hold_bound(kind, b["in"], b["out"].cpu(), lp, lp, "sampler")
    assert torch.equal(b["in"], D.resample(b["out"], lp, kind))


@pytest.mark.parametrize("kind", NEW_KINDS)
def test_make_test_pair_with_a_degradation(kind):
    hr = torch.rand(2, 1, 44, 40, generator=torch.Generator().manual_seed(4)).to(DEV)
    lr, gt, rs = D.make_test_pair(hr, 4, kind)
    lr0, gt0, rs0 = D.make_test_pair(hr, 4)
    assert lr.shape == (2, 1, 11, 10) and torch.equal(lr, D.resample(hr, (11, 10), kind)) and not torch.equal(lr, lr0)
    assert gt is hr and gt0 is hr and rs == rs0 == (4.0, 4.0)
    lr, gt, rs = D.make_test_pair(hr, 3, D.Degradation(kind))          # 14 x 13 -> gt 42 x 39: the plain cubic resize
    lr0, gt0, rs0 = D.make_test_pair(hr, 3)
    assert torch.equal(lr, D.resample(hr, (14, 13), kind)) and torch.equal(gt, gt0) and rs == rs0
    assert torch.equal(D.make_test_pair(hr, 3, "cubic")[0], lr0)


def test_step_from_with_a_blurring_sampler_under_the_graph():
    """step_from(sampler) with 'cubic+gaussian' against step(b['in'], b['out']) on the batches sample(draw=) gives for the same
    draws: two eager steps, the capture, two replays that sample straight into the graph's tensors; the same losses bit for
    bit.  sample() must not wait for the device (the tables are resident after the first batch).  Bias tables frozen as in
    tests/test_data_gpu.py::test_step_from_is_step_on_the_same_batches, for its reason."""
    from rdst_amd.trainer import DPTrainStep
    imgs, _ = _stack(5, 1, 80, 72, seed=9)
    res = {}
    for via in ("step", "step_from"):
        net = _net("bf16")
        for name, prm in net.named_parameters():
            if name.endswith("relative_position_bias_table"):
                prm.requires_grad_(False)
        tr = DPTrainStep(net, lr=1e-3, graph=True, graph_warmup=2)
        s = D.DevicePatchSampler(imgs, 2, 16, sr_scales=(4.0,), device=DEV, generator=torch.Generator().manual_seed(21),
                                 degradation="cubic+gaussian")
        losses, in_place = [], []
        for i in range(5):
            if via == "step":
                draw = s.draw()
                torch.cuda.set_sync_debug_mode("error" if i else "default")
                try:
                    b = s.sample(draw=draw)
                finally:
                    torch.cuda.set_sync_debug_mode("default")
                assert torch.equal(b["in"], D.resample(b["out"], 16, "cubic+gaussian"))
                losses.append(tr.step(b["in"], b["out"]).clone())
            else:
                losses.append(tr.step_from(s).clone())
                b = tr.last_batch
                assert b["degradation"] == D.Degradation("cubic+gaussian") and b["in"].shape == (2, 1, 16, 16)
                in_place.append(tr._static is not None and b["in"].data_ptr() == tr._static[0].data_ptr()
                                and b["out"].data_ptr() == tr._static[1].data_ptr())
        torch.cuda.synchronize()
        assert tr.graph is not None
        if via == "step_from":
            assert in_place == [False] * 3 + [True] * 2
        res[via] = [l.item() for l in losses]
    assert res["step"] == res["step_from"]
