"""GPU: DPTrainStep.quick_eva, the reference trainer's quick validation (models/basic_trainer.py:257-286), on the tiny
network of smoke(): its report against numpy scoring of the same reconstructions, and a training run that it must leave
bit for bit as it was (eager and graph-replayed steps)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import rdst_oracle as O
from rdst_amd import metrics as M
from rdst_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = {"psnr": 1e-9, "ssim": 1e-10}


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


def _validation_set(n=12, h=16, w=24, seed=2):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 1, h, w, generator=g), torch.rand(n, 1, 4 * h, 4 * w, generator=g)


def _reference_report(net, lr, hr, seed, num_samples, batch_size, mode):
    """What quick_eva must compute, spelled out: the same slices, the same chunks, numpy scoring."""
    idx = torch.randperm(len(lr), generator=torch.Generator().manual_seed(seed))[:num_samples]
    was = net.training
    net.eval()
    with torch.no_grad():
        rec = torch.cat([net(p.to(DEV)) for p in lr[idx].split(batch_size * 4)])
    net.train(was)
    rep = M.SRMetrics("psnr ssim", mode)(hr[idx], rec, 4)
    return {f"{m}_4.0": v for m, v in rep.items()}


def _close(got, want):
    assert list(got) == list(want)
    for k, v in want.items():
        tol = TOL[k.split("_")[0]]
        assert np.allclose(got[k], v, rtol=0, atol=tol), (k, got[k], v)


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp32x3"])
def test_report_matches_numpy_scoring(mode):
    from rdst_amd.trainer import DPTrainStep
    net = _net(mode)
    code = net.compute_code
    tr = DPTrainStep(net, lr=1e-3)
    lr, hr = _validation_set()
    rep = tr.quick_eva(lr, hr, num_samples=8, batch_size=1, generator=torch.Generator().manual_seed(11))
    assert tr.quick_validation_reports == [rep] and set(rep) == {"psnr_4.0", "ssim_4.0"}
    assert all(isinstance(v, float) and math.isfinite(v) for v in rep.values())
    _close(rep, _reference_report(net, lr, hr, 11, 8, 1, "mean"))
    full = tr.quick_eva(lr.to(DEV), hr, sr_scale=4, metrics="ssim psnr", num_samples=5, batch_size=2,
                        generator=torch.Generator().manual_seed(3), return_mode="full")
    assert list(full) == ["ssim_4.0", "psnr_4.0"] and len(full["psnr_4.0"]) == 5
    _close(full, {k: _reference_report(net, lr, hr, 3, 5, 2, "full")[k] for k in full})
    assert len(tr.quick_validation_reports) == 2 and net.training and net.compute_code == code


def test_restores_training_flags():
    from rdst_amd.trainer import DPTrainStep
    net = _net()
    tr = DPTrainStep(net)
    lr, hr = _validation_set(n=4)
    net.tail.eval()                       # a submodule the caller keeps in eval mode stays so
    flags = [m.training for m in net.modules()]
    tr.quick_eva(lr, hr, num_samples=2)
    assert [m.training for m in net.modules()] == flags
    net.eval()
    tr.quick_eva(lr, hr, num_samples=2)
    assert not any(m.training for m in net.modules())
    with pytest.raises(ValueError):
        tr.quick_eva(lr, hr, metrics="psnr fid")
    assert len(tr.quick_validation_reports) == 2


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_training_run_unchanged(graph):
    """Six steps with a quick validation after steps 2 and 4 give the losses and parameters of six steps without it, bit for
    bit; in the graph run the first call falls between the eager warm-up and the capture, the second between replays.
    The relative-position bias tables are frozen here: the attention backward sums their gradient with LDS float atomics
    (csrc/wattn_bwd_mfma.hip), so two runs of the same steps differ in its last bits whether or not quick_eva runs between
    them; every other gradient of this network has a fixed summation order, which makes the comparison bitwise."""
    from rdst_amd.trainer import DPTrainStep
    g = torch.Generator().manual_seed(5)
    data = [(torch.rand(2, 1, 16, 16, generator=g).to(DEV), torch.rand(2, 1, 64, 64, generator=g).to(DEV)) for _ in range(6)]
    lr, hr = _validation_set(n=6, h=16, w=16)
    res = {}
    for with_eva in (False, True):
        net = _net("bf16")
        for name, prm in net.named_parameters():
            if name.endswith("relative_position_bias_table"):
                prm.requires_grad_(False)
        tr = DPTrainStep(net, lr=1e-3, graph=graph, graph_warmup=2)
        losses = []
        for i, (x, t) in enumerate(data):
            losses.append(tr.step(x, t).clone())
            if with_eva and i in (1, 3):
                plan = ops.pack_plan_of(net)          # the packed weights the steps (and a captured graph) use, if any
                tr.quick_eva(lr, hr, num_samples=4, batch_size=1, generator=torch.Generator().manual_seed(i))
                assert ops.pack_plan_of(net) is plan
        torch.cuda.synchronize()
        assert (tr.graph is not None) == graph
        assert len(tr.quick_validation_reports) == (2 if with_eva else 0)
        res[with_eva] = ([l.item() for l in losses], tr.optimizer.flat_param.clone(), tr.loss_records()["L1"])
    assert res[False][0] == res[True][0]
    assert torch.equal(res[False][1], res[True][1])
    assert res[False][2] == res[True][2] == res[False][0]


def test_checkpoint_round_trips_the_reports(tmp_path):
    from rdst_amd.trainer import DPTrainStep
    net = _net()
    tr = DPTrainStep(net, lr=1e-3)
    lr, hr = _validation_set(n=6)
    tr.step(F.interpolate(hr[:2], scale_factor=0.25).to(DEV), hr[:2].to(DEV))
    for seed in (1, 2):
        tr.quick_eva(lr, hr, num_samples=3, generator=torch.Generator().manual_seed(seed))
    path = str(tmp_path / "checkpoint.tar")
    tr.save_checkpoint(path)
    other = DPTrainStep(_net(), lr=1e-3)
    other.load_checkpoint(path)
    assert other.quick_validation_reports == tr.quick_validation_reports and len(other.quick_validation_reports) == 2
    other.quick_eva(lr, hr, num_samples=3)
    assert len(other.quick_validation_reports) == 3
