"""GPU: rdst_amd.data — the HIP bicubic resize against torch's float64 bicubic on the CPU (the oracle: it equals the closed
form, tests/test_data_host.py), the one-launch patch sampler against slicing and the resize, make_test_pair against the
oracle and through SRTester, and DPTrainStep.step_from against step() on the same batches (eager and graph-replayed)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import rdst_oracle as O
from rdst_amd import data as D
from rdst_amd import metrics as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

SIZE_PAIRS = [((96, 96), (24, 24)), ((256, 256), (64, 64)), ((176, 208), (44, 52)), ((160, 200), (64, 80)),
              ((100, 90), (66, 60)), ((44, 52), (176, 208)), ((97, 131), (27, 37))]
# Inputs in [0, 1]; the largest sum of |tap weights| of an axis is 1.375 (at fraction 0.5); 24 fp32 roundings (the weights,
# two 4-tap passes, the intermediate) bound the error by 24 * 2^-24 * 1.375^2 = 2.7e-6.
TOL = 3e-6


def _oracle(x, size):
    return F.interpolate(x.detach().cpu().double(), size=size, mode="bicubic", align_corners=False)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("src,dst", SIZE_PAIRS)
def test_resize_matches_float64_bicubic(src, dst, C):
    x = torch.rand(2, C, *src, generator=torch.Generator().manual_seed(src[0] + dst[1] + C))
    y = D.bicubic_resize(x.to(DEV), dst)
    assert y.shape == (2, C, *dst) and y.dtype == torch.float32 and y.device == DEV
    err = (y.cpu().double() - _oracle(x, dst)).abs().max().item()
    print(f"[resize] {src} -> {dst} C={C}: max|d| = {err:.3e}")
    assert err <= TOL
    # an int is a square size; a (C, H, W) image comes back as one
    y3 = D.bicubic_resize(x[0].to(DEV), dst)
    assert torch.equal(y3, y[0])


def test_resize_of_an_impulse_is_exact():
    """hp = 4 lp: the taps are -3/32, 19/32, 19/32, -3/32 and every product of two of them is a dyadic rational."""
    k = np.array([-3 / 32, 19 / 32, 19 / 32, -3 / 32])
    for (r, c) in [(0, 0), (21, 38), (63, 63), (30, 1)]:
        x = torch.zeros(1, 1, 64, 64)
        x[0, 0, r, c] = 1.0
        want = np.zeros((16, 16))
        want[r // 4, c // 4] = k[r % 4] * k[c % 4]
        y = D.bicubic_resize(x.to(DEV), 16)
        assert np.array_equal(y[0, 0].cpu().double().numpy(), want)
        assert np.float32(want[r // 4, c // 4]) == want[r // 4, c // 4]


def test_resize_refuses():
    x = torch.rand(1, 1, 8, 8, device=DEV)
    with pytest.raises(RuntimeError):
        D.bicubic_resize(x.clone().requires_grad_(True), 4)
    with pytest.raises(RuntimeError):
        D.bicubic_resize(x.cpu(), 4)
    with pytest.raises(TypeError):
        D.bicubic_resize(x.double(), 4)
    with pytest.raises(ValueError):
        D.bicubic_resize(x, (0, 4))


def _stack(S, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(S, C, H, W, generator=g), torch.randint(0, 5, (S, H, W), generator=g, dtype=torch.uint8)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("scale,shape", [(4.0, (70, 90)), (4.0, (50, 90)), (3.0, (70, 90)), (2.0, (70, 90)), (2.5, (70, 90))],
                         ids=["x4", "x4-padded", "x3", "x2", "x2.5"])
def test_sampler_batches(scale, shape, C):
    S, B, lp = 12, 8, 16
    hp = int(lp * scale)
    imgs, labels = _stack(S, C, *shape, seed=int(10 * scale) + C)

    def sampler(seed):
        return D.DevicePatchSampler(imgs, B, lp, sr_scales=(scale,), labels=labels, device=DEV,
                                    generator=torch.Generator().manual_seed(seed))
    s = sampler(3)
    assert (s.H, s.W) == (max(shape[0], hp), shape[1])
    padded, plabels = D.edge_pad(imgs, hp), D.edge_pad(labels, hp)
    assert torch.equal(s.hr_images.cpu(), padded) and torch.equal(s.labels.cpu(), plabels)
    other = sampler(3)
    for it in range(3):
        b = s.sample()
        idx = b["indices"]
        assert set(b) == {"in", "out", "sr_factor", "real_sr_scale", "indices", "label"}
        assert b["sr_factor"] == scale and b["real_sr_scale"] == hp / lp
        assert not idx.is_cuda and tuple(idx.shape) == (B, 3) and len(set(idx[:, 0].tolist())) == B
        assert b["out"].shape == (B, C, hp, hp) and b["in"].shape == (B, C, lp, lp)
        assert b["label"].shape == (B, 1, hp, hp) and b["label"].dtype == torch.int64
        for k, (sl, top, left) in enumerate(idx.tolist()):
            assert torch.equal(b["out"][k].cpu(), padded[sl, :, top:top + hp, left:left + hp])
            assert torch.equal(b["label"][k, 0].cpu(), plabels[sl, top:top + hp, left:left + hp].long())
        err = (b["in"].cpu().double() - _oracle(b["out"], (lp, lp))).abs().max().item()
        print(f"[sampler] x{scale} C={C} batch {it}: max|d| = {err:.3e}")
        assert err <= TOL
        assert torch.equal(b["in"], D.bicubic_resize(b["out"], lp))
        o = other.sample()
        assert torch.equal(o["indices"], idx) and torch.equal(o["in"], b["in"]) and torch.equal(o["out"], b["out"])
        assert torch.equal(o["label"], b["label"])
    # into tensors the caller owns
    lr, hr = torch.zeros(B, C, lp, lp, device=DEV), torch.zeros(B, C, hp, hp, device=DEV)
    b = s.sample(out=(lr, hr))
    o = other.sample()
    assert b["in"] is lr and b["out"] is hr
    assert torch.equal(lr, o["in"]) and torch.equal(hr, o["out"])
    with pytest.raises(ValueError):
        s.sample(out=(hr, lr))


@pytest.mark.parametrize("scale", [4.0, 2.0], ids=["x4", "x2"])
def test_kernel_clamps_origins_it_was_not_promised(scale):
    """The index table is device memory the host never reads: slice, top and left outside the stack give the nearest
    window inside it.  The stack is a view in the middle of a larger zero buffer here, so that even an unclamped
    origin of this size would stay inside the allocation."""
    S, B, lp, H, W = 6, 4, 8, 40, 48
    hp = int(lp * scale)
    imgs, labels = _stack(S, 2, H, W, seed=5)
    s = D.DevicePatchSampler(imgs, B, lp, sr_scales=(scale,), labels=labels, device=DEV)
    big = torch.zeros(S + 8, 2, H, W, device=DEV)
    big[4:4 + S] = s.hr_images
    bigl = torch.zeros(S + 8, H, W, dtype=torch.uint8, device=DEV)
    bigl[4:4 + S] = s.labels
    s.hr_images, s.labels = big[4:4 + S], bigl[4:4 + S]
    wild = torch.tensor([[S + 2, -3, W - hp + 5], [-2, H, -1], [2, H - hp + 1, 7], [S, 3, W]], dtype=torch.int32)
    b = s.sample(draw=D.Draw(scale, hp, wild))
    for k, (sl, top, left) in enumerate(wild.tolist()):
        sl, top, left = min(max(sl, 0), S - 1), min(max(top, 0), H - hp), min(max(left, 0), W - hp)
        assert torch.equal(b["out"][k].cpu(), imgs[sl, :, top:top + hp, left:left + hp])
        assert torch.equal(b["label"][k, 0].cpu(), labels[sl, top:top + hp, left:left + hp].long())
    assert torch.equal(b["in"], D.bicubic_resize(b["out"], lp))


@pytest.mark.parametrize("lp", [120, 121], ids=["hp240-wide", "hp242-scalar"])
def test_wide_patches_where_the_two_4tap_entries_band_differently(lp):
    """rdst_sample_patches and rdst_sample_patches_d8 share one host plan and differ in its LDS budget: the transposing block
    of the second takes 5376 bytes of the 64 KB.  At ratio 2 a band of 32 LR rows stages 67 HR rows, which fit the whole
    budget up to hp = 244 (67 hp 4 <= 65536) and the reduced one up to hp = 224, so at hp = 240 and 242 the plain entry cuts
    bands of 32 rows and the d8 entry bands of 16: other bands, the same batch."""
    S, B, hp = 3, 2, 2 * lp
    imgs, labels = _stack(S, 1, 250, 260, seed=lp)
    s = D.DevicePatchSampler(imgs, B, lp, sr_scales=(2.0,), labels=labels, device=DEV, generator=torch.Generator().manual_seed(1))
    d = s.draw()
    b = s.sample(draw=d)
    for k, (sl, top, left) in enumerate(d.indices.tolist()):
        assert torch.equal(b["out"][k].cpu(), imgs[sl, :, top:top + hp, left:left + hp])
        assert torch.equal(b["label"][k, 0].cpu(), labels[sl, top:top + hp, left:left + hp].long())
    assert torch.equal(b["in"], D.bicubic_resize(b["out"], lp))
    t = s.sample(draw=d._replace(variants=torch.zeros(B, dtype=torch.int32)))
    assert torch.equal(t["in"], b["in"]) and torch.equal(t["out"], b["out"]) and torch.equal(t["label"], b["label"])


def test_sampler_without_labels_and_with_several_scales():
    imgs, _ = _stack(6, 1, 40, 48, seed=2)
    s = D.DevicePatchSampler([a.permute(1, 2, 0).numpy() for a in imgs], 4, 8, sr_scales=(2.0, 3.0, 4.0), device=DEV,
                             generator=torch.Generator().manual_seed(0))
    seen = set()
    for _ in range(16):
        b = s.sample()
        hp = int(8 * b["sr_factor"])
        seen.add(b["sr_factor"])
        assert "label" not in b and b["out"].shape == (4, 1, hp, hp)
        for k, (sl, top, left) in enumerate(b["indices"].tolist()):
            assert torch.equal(b["out"][k].cpu(), imgs[sl, :, top:top + hp, left:left + hp])
        assert (b["in"].cpu().double() - _oracle(b["out"], (8, 8))).abs().max().item() <= TOL
    assert seen == {2.0, 3.0, 4.0}


def _net(mode="fp32"):
    from rdst_amd.networks.rdst_variations import RDSTSR
    cfg = O.make_cfg(**{**O.CFG_TINY, "img_size": 16})
    net = RDSTSR(img_size=16, in_chans=1, sr_scale=4, embed_dim=48, dense_layer_depths=[2, 2], num_heads=[6, 6],
                 window_size=[8, 8], rdb_depths=[3, 3], mlp_ratio=2.0, growth_rate=24, pre_norm=True,
                 feature_last_operation=True)
    net.load_state_dict(O.make_weights(cfg, 7), strict=True)
    net.to(DEV).train()
    if mode != "fp32":
        net.set_compute_dtype(mode)
    return net


def test_make_test_pair():
    g = torch.Generator().manual_seed(4)
    hr = torch.rand(2, 1, 176, 208, generator=g)
    lr, gt, rs = D.make_test_pair(hr.to(DEV), 4)
    assert lr.shape == (2, 1, 44, 52) and rs == (4.0, 4.0)
    assert torch.equal(gt.cpu(), hr)
    assert (lr.cpu().double() - _oracle(hr, (44, 52))).abs().max().item() <= TOL
    hr = torch.rand(2, 3, 97, 131, generator=g)
    lr, gt, rs = D.make_test_pair(hr.to(DEV), 2.5)
    assert lr.shape == (2, 3, 38, 52) and gt.shape == (2, 3, 95, 130) and rs == (95 / 38, 130 / 52)
    assert (lr.cpu().double() - _oracle(hr, (38, 52))).abs().max().item() <= TOL
    assert (gt.cpu().double() - _oracle(hr, (95, 130))).abs().max().item() <= TOL


def test_test_pair_feeds_the_tester():
    from rdst_amd.tester import SRTester
    net = _net()
    hr = torch.rand(6, 1, 160, 192, generator=torch.Generator().manual_seed(6)).to(DEV)
    lr, gt, rs = D.make_test_pair(hr, 4)
    assert lr.shape == (6, 1, 40, 48) and gt is hr and rs == (4.0, 4.0)
    rep = SRTester(net, batch_size=1).evaluate(lr, gt, on_device=True)
    net.eval()
    with torch.no_grad():
        rec = torch.cat([net(p) for p in lr.split(4)])
    mse, ssim = (t.cpu().tolist() for t in M.device_scores(gt, rec, 4))
    assert rep["psnr"] == [M.psnr_from_mse(v) for v in mse] and rep["ssim"] == ssim


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_step_from_is_step_on_the_same_batches(graph):
    """Six steps through step_from(sampler) against six step(b['in'], b['out']) fed by a second sampler with the same seed:
    the same losses and parameters, bit for bit.  The relative-position bias tables are frozen as in
    tests/test_quick_eva_gpu.py::test_training_run_unchanged and for its reason: their gradient is summed with LDS float
    atomics, so two runs of the same steps differ in its last bits anyway."""
    from rdst_amd.trainer import DPTrainStep
    imgs, _ = _stack(5, 1, 80, 72, seed=9)
    res = {}
    for via in ("step", "step_from"):
        net = _net("bf16")
        for name, prm in net.named_parameters():
            if name.endswith("relative_position_bias_table"):
                prm.requires_grad_(False)
        tr = DPTrainStep(net, lr=1e-3, graph=graph, graph_warmup=2)
        s = D.DevicePatchSampler(imgs, 2, 16, sr_scales=(4.0,), device=DEV, generator=torch.Generator().manual_seed(21))
        losses, in_place = [], []
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
        torch.cuda.synchronize()
        assert (tr.graph is not None) == graph
        if via == "step_from":       # two eager steps, the capturing step on a fresh batch, then straight into the graph's tensors
            assert in_place == ([False] * 3 + [True] * 3 if graph else [False] * 6)
        res[via] = ([l.item() for l in losses], tr.optimizer.flat_param.clone())
    assert res["step"][0] == res["step_from"][0]
    assert torch.equal(res["step"][1], res["step_from"][1])
