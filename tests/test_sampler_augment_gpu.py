"""GPU: the sampler's augmentation (DevicePatchSampler(augment=...), rdst_sample_patches_d8).  Crop, then transform, then
degrade: the HR patches and label crops of a batch against tiling.dihedral of the plain sampler's for the same origins, the LR
patches against bicubic_resize of the transformed HR patches, on every path of the entry point; what the kernel does with
variants outside 0..7; the free-running sampler; and DPTrainStep.step_from on an augmenting sampler against step() on the same
batches.  Every assertion is torch.equal: the accuracy of the resize itself is gated in tests/test_data_gpu.py."""
import pytest
import torch

from rdst_amd import data as D
from rdst_amd.tiling import dihedral
from test_data_gpu import _net, _stack

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
S, B = 8, 8

# (scale, lp, the outputs at an address that is 4-byte but not 16-byte aligned)
PATHS = {
    "x4-lp6": (4.0, 6, False),         # the ratio-4 path, one partial 32 x 32 block per plane
    "x4-lp16": (4.0, 16, False),       # the ratio-4 path, whole blocks
    "x4-unaligned": (4.0, 6, True),    # ratio 4 on the scalar table path
    "x2-lp8": (2.0, 8, False),         # the table path, 16-byte flavour
    "x3-lp5": (3.0, 5, False),         # hp = 15: scalar
    "x2.5-lp6": (2.5, 6, False),       # hp = 15: scalar, a fractional ratio
    "x2-lp40": (2.0, 40, False),       # hp = 80: two bands of LR rows, blocks partial in both directions
}


def _setup(scale, lp, C, seed=11):
    """A non-square stack a little larger than the patch (never padded), labels, and origins that touch both corners."""
    hp = int(lp * scale)
    H, W = max(40, hp + 7), max(52, hp + 19)
    imgs, labels = _stack(S, C, H, W, seed=seed)
    s = D.DevicePatchSampler(imgs, B, lp, sr_scales=(scale,), labels=labels, device=DEV)
    assert (s.H, s.W) == (H, W)
    g = torch.Generator().manual_seed(seed)
    idx = torch.stack([torch.randperm(S, generator=g), torch.randint(0, H - hp + 1, (B,), generator=g),
                       torch.randint(0, W - hp + 1, (B,), generator=g)], dim=1).to(torch.int32)
    idx[0, 1:] = 0
    idx[1, 1], idx[1, 2] = H - hp, W - hp
    idx[2, 1], idx[2, 2] = 0, W - hp
    return s, imgs, labels, idx, hp


def _odd_outs(B, C, lp, hp):
    """Contiguous (inputs, targets) one float past a 16-byte boundary."""
    lr = torch.zeros(B * C * lp * lp + 1, device=DEV)[1:].view(B, C, lp, lp)
    hr = torch.zeros(B * C * hp * hp + 1, device=DEV)[1:].view(B, C, hp, hp)
    assert hr.data_ptr() % 16 == 4 and lr.data_ptr() % 16 == 4
    return lr, hr


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("path", list(PATHS))
def test_every_transform_on_every_path(path, C):
    scale, lp, odd = PATHS[path]
    s, imgs, labels, idx, hp = _setup(scale, lp, C)
    plain = s.sample(draw=D.Draw(scale, hp, idx))
    assert "variants" not in plain
    for b, (sl, top, left) in enumerate(idx.tolist()):           # the plain batch is the crops themselves
        assert torch.equal(plain["out"][b].cpu(), imgs[sl, :, top:top + hp, left:left + hp])
        assert torch.equal(plain["label"][b, 0].cpu(), labels[sl, top:top + hp, left:left + hp].long())
    variants = torch.arange(8, dtype=torch.int32)
    out = _odd_outs(B, C, lp, hp) if odd else None
    b8 = s.sample(out=out, draw=D.Draw(scale, hp, idx, variants))
    assert set(b8) == set(plain) | {"variants"} and torch.equal(b8["variants"], variants) and b8["indices"] is idx
    if odd:
        assert b8["in"] is out[0] and b8["out"] is out[1]
    assert b8["out"].shape == (B, C, hp, hp) and b8["in"].shape == (B, C, lp, lp) and b8["label"].shape == (B, 1, hp, hp)
    for b in range(B):
        assert torch.equal(b8["out"][b], dihedral(plain["out"][b], b)), (path, b)
        assert torch.equal(b8["label"][b], dihedral(plain["label"][b], b)), (path, b)
    assert torch.equal(b8["in"], D.bicubic_resize(b8["out"].contiguous(), lp))
    # no atomics: the same bits again
    again = s.sample(draw=D.Draw(scale, hp, idx, variants))
    assert torch.equal(again["in"], b8["in"]) and torch.equal(again["out"], b8["out"]) and torch.equal(again["label"], b8["label"])


@pytest.mark.parametrize("path", ["x4-lp16", "x4-unaligned", "x2-lp8", "x3-lp5"])
def test_all_zero_variants_are_the_plain_batch(path):
    scale, lp, odd = PATHS[path]
    s, _, _, idx, hp = _setup(scale, lp, 2, seed=13)
    plain = s.sample(out=_odd_outs(B, 2, lp, hp) if odd else None, draw=D.Draw(scale, hp, idx))
    zero = s.sample(out=_odd_outs(B, 2, lp, hp) if odd else None, draw=D.Draw(scale, hp, idx, torch.zeros(B, dtype=torch.int32)))
    for key in ("in", "out", "label"):
        assert torch.equal(zero[key], plain[key]), key


def test_the_same_seed_gives_the_same_augmented_batches():
    imgs, labels = _stack(10, 2, 40, 52, seed=3)

    def sampler():
        return D.DevicePatchSampler(imgs, 4, 6, sr_scales=(2.0, 4.0), labels=labels, device=DEV, augment=True,
                                    generator=torch.Generator().manual_seed(17))
    a, b = sampler(), sampler()
    for _ in range(4):
        x, y = a.sample(), b.sample()
        assert x["sr_factor"] == y["sr_factor"]
        for key in ("indices", "variants", "in", "out", "label"):
            assert torch.equal(x[key], y[key]), key


@pytest.mark.parametrize("scale", [4.0, 2.0], ids=["x4", "x2"])
def test_kernel_masks_variants_it_was_not_promised(scale):
    """The variant table is device memory the host never reads: the kernel takes k & 7.  The stack is a view in the middle of
    a larger zero buffer, as in tests/test_data_gpu.py::test_kernel_clamps_origins_it_was_not_promised."""
    lp = 8
    s, _, _, idx, hp = _setup(scale, lp, 2, seed=5)
    big = torch.zeros(S + 8, 2, s.H, s.W, device=DEV)
    big[4:4 + S] = s.hr_images
    bigl = torch.zeros(S + 8, s.H, s.W, dtype=torch.uint8, device=DEV)
    bigl[4:4 + S] = s.labels
    s.hr_images, s.labels = big[4:4 + S], bigl[4:4 + S]
    wild = torch.tensor([11, 21, 8, 30, -1, 12, -6, (1 << 20) + 1], dtype=torch.int32)
    tame = torch.tensor([3, 5, 0, 6, 7, 4, 2, 1], dtype=torch.int32)
    assert torch.equal(wild & 7, tame)
    a = s.sample(draw=D.Draw(scale, hp, idx, wild))
    b = s.sample(draw=D.Draw(scale, hp, idx, tame))
    for key in ("in", "out", "label"):
        assert torch.equal(a[key], b[key]), key
    assert torch.equal(a["variants"], wild)
    assert torch.equal(a["out"][0], dihedral(s.sample(draw=D.Draw(scale, hp, idx))["out"][0], 3))


def test_free_running_sampler_reports_what_it_did():
    imgs, labels = _stack(12, 2, 40, 52, seed=8)
    lp, hp = 6, 24
    s = D.DevicePatchSampler(imgs, 4, lp, sr_scales=(4.0,), labels=labels, device=DEV, augment=True,
                             generator=torch.Generator().manual_seed(0))
    seen = set()
    for _ in range(16):
        b = s.sample()
        assert set(b) == {"in", "out", "sr_factor", "real_sr_scale", "indices", "label", "variants"}
        idx, var = b["indices"], b["variants"]
        assert tuple(idx.shape) == (4, 3) and not idx.is_cuda and len(set(idx[:, 0].tolist())) == 4
        assert tuple(var.shape) == (4,) and var.dtype == torch.int32 and not var.is_cuda
        for k, ((sl, top, left), v) in enumerate(zip(idx.tolist(), var.tolist())):
            assert torch.equal(b["out"][k].cpu(), dihedral(imgs[sl, :, top:top + hp, left:left + hp], v))
            assert torch.equal(b["label"][k, 0].cpu(), dihedral(labels[sl, top:top + hp, left:left + hp], v).long())
        assert torch.equal(b["in"], D.bicubic_resize(b["out"], lp))
        seen |= set(var.tolist())
    assert seen == set(range(8))
    # forced variants need the batch's length and integers
    d = s.draw()
    with pytest.raises(ValueError):
        s.sample(draw=D.Draw(d.sr_factor, d.hr_patch_size, d.indices, torch.zeros(3, dtype=torch.int32)))
    with pytest.raises(ValueError):
        s.sample(draw=D.Draw(d.sr_factor, d.hr_patch_size, d.indices, torch.zeros(4)))


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_step_from_an_augmenting_sampler_is_step_on_the_same_batches(graph):
    """tests/test_data_gpu.py::test_step_from_is_step_on_the_same_batches with augment=True (and labels): six steps through
    step_from(sampler) against six step(b['in'], b['out']) fed by a twin sampler, the same losses and parameters bit for bit,
    the bias tables frozen for the reason given there.  After the capture the augmented batch is written straight into the
    graph's tensors; last_batch keeps the variants and the labels, transformed like their patch."""
    from rdst_amd.trainer import DPTrainStep
    imgs, labels = _stack(5, 1, 80, 72, seed=9)
    res = {}
    for via in ("step", "step_from"):
        net = _net("bf16")
        for name, prm in net.named_parameters():
            if name.endswith("relative_position_bias_table"):
                prm.requires_grad_(False)
        tr = DPTrainStep(net, lr=1e-3, graph=graph, graph_warmup=2)
        s = D.DevicePatchSampler(imgs, 2, 16, sr_scales=(4.0,), labels=labels, device=DEV, augment=True,
                                 generator=torch.Generator().manual_seed(21))
        losses, in_place, variants = [], [], []
        for i in range(6):
            if via == "step":
                b = s.sample()
                losses.append(tr.step(b["in"], b["out"]).clone())
            else:
                losses.append(tr.step_from(s).clone())
                b = tr.last_batch
                assert b["in"].shape == (2, 1, 16, 16) and b["out"].shape == (2, 1, 64, 64)
                in_place.append(tr._static is not None and b["in"].data_ptr() == tr._static[0].data_ptr()
                                and b["out"].data_ptr() == tr._static[1].data_ptr())
            variants.append(b["variants"].clone())
        torch.cuda.synchronize()
        assert (tr.graph is not None) == graph
        if via == "step_from":
            assert in_place == ([False] * 3 + [True] * 3 if graph else [False] * 6)
            for k, ((sl, top, left), v) in enumerate(zip(b["indices"].tolist(), b["variants"].tolist())):
                assert torch.equal(b["out"][k].cpu(), dihedral(imgs[sl, :, top:top + 64, left:left + 64], v))
                assert torch.equal(b["label"][k, 0].cpu(), dihedral(labels[sl, top:top + 64, left:left + 64], v).long())
        res[via] = ([l.item() for l in losses], tr.optimizer.flat_param.clone(), torch.stack(variants))
    assert torch.equal(res["step"][2], res["step_from"][2]) and len(set(res["step"][2].flatten().tolist())) > 1
    assert res["step"][0] == res["step_from"][0]
    assert torch.equal(res["step"][1], res["step_from"][1])
