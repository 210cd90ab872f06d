"""Every call rdst_amd/ops.py makes through the C ABI, in order and with its arguments, against a recorded trace
(tests/golden/ops_call_trace.json): the pin under which the host side above the ABI is refactored.  No GPU: the library is
replaced by a recording stand-in that answers 0 (or ENOTSUP where a scenario scripts a refusal) and forwards only the pure
host queries (*_packable, *_supported, *_workspace, *_workspace2) to the real library, which loads without a device - with
made-up sizes the K8 image split degenerates.  Autograd, PackPlan recording and reuse, the reduction batches and the dense-join
sink all run on CPU tensors; ``_lib.load``, ``ops._need_gpu`` and ``ops._stream`` are the only things patched.

One record per call, arguments in ABI order: numbers verbatim, PREPACKED as a word, pointers (positions from _lib.SIGNATURES)
as ``null``, ``<parameter>[+<byte offset>]`` inside a parameter of the scenario's module, ``arena+<offset>`` inside its plan
arena, ``grads+<offset>`` inside its flat gradient bucket, else ``buf<k>`` - k numbers the distinct other addresses WITHIN
that call, so aliasing between a call's arguments is pinned and allocator reuse is not.  rdst_pack_batch is followed by its
decoded job table.  ``plan:`` lines give the module's PackPlan after a forward.  The scenarios repeat most of their records
(the same network, step after step), so the file keeps each distinct record once and a scenario as a list of indices into them.

Not covered here: the ``g.is_cuda`` branch of _DenseJoin.backward (the layer's outer reduction batch does not open on CPU
tensors; one scenario opens a batch by hand instead) and real refusals by the kernels.  The GPU suite covers both:
test_grad_accum_gpu.py, test_mlp_gpu.py::test_swin_block_backward_with_misaligned_gradient, test_lnlin3_gpu.py.
The stand-in answers 0 and writes nothing, so the frozen-parameter scenarios pin only WHICH calls are made (and with which
NULL outputs); what those calls compute is checked in test_partial_grads_gpu.py, which runs the same freeze patterns through
ops.swin_block and every NULL pattern of rdst_ln_linear_bwd / rdst_conv_bwd on the device against float64 autograd.

    python tests/test_ops_trace.py --record   # rewrite the trace from the rdst_amd/ops.py in the tree
"""
import collections
import ctypes
import json
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from rdst_amd import _lib, dp, ops  # noqa: E402
from rdst_amd.networks.rdst_variations import RDSTSR, _apply_res_connection  # noqa: E402
from rdst_amd.networks.swin_transformer_sr import SwinTransformerBlock, WindowAttention, _norm_only  # noqa: E402

TRACE = os.path.join(HERE, "golden", "ops_call_trace.json")
QUERIES = ("_packable", "_supported", "_workspace", "_workspace2")
REAL_LOAD = _lib.load


class Recorder:
    """What ``_lib.load()`` returns during a scenario."""

    def __init__(self, named=lambda: (), owner=None, refuse=None):
        self.real = REAL_LOAD()
        self.named, self.owner = named, owner     # () -> (name, tensor) pairs of the scenario; the module whose plan arena counts
        self.refuse = refuse or {}                # name -> the 1-based calls of that name which answer ENOTSUP
        self.seen = collections.Counter()
        self.lines = []
        self.bucket = None

    def label(self, addr, bufs):
        if isinstance(addr, ctypes.c_void_p):
            addr = addr.value
        if not addr:
            return "null"
        regions = list(self.named())
        plan = ops.pack_plan_of(self.owner) if self.owner is not None else None
        if plan is not None and plan.arena is not None:
            regions.append(("arena", plan.arena))
        if self.bucket is not None:
            regions.append(("grads", self.bucket.flat))
        for name, t in regions:
            off = addr - t.data_ptr()
            if 0 <= off < max(t.numel() * t.element_size(), 1):
                return f"{name}+{off}" if off else name
        return f"buf{bufs.setdefault(addr, len(bufs))}"

    def __getattr__(self, name):
        if name.endswith(QUERIES):
            return getattr(self.real, name)
        if name == "rdst_last_error":
            return lambda: b"scripted"
        argtypes = _lib.SIGNATURES[name][1]

        def call(*args):
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            bufs, out = {}, []
            for a, ty in zip(args, argtypes):
                if ty is ctypes.c_void_p:
                    out.append("jobs" if name == "rdst_pack_batch" and not out else self.label(a, bufs))
                elif ty is ctypes.c_size_t and a == _lib.PREPACKED:
                    out.append("PREPACKED")
                else:
                    out.append(repr(float(a)) if isinstance(a, float) else str(int(a)))
            self.lines.append(f"{name}({', '.join(out)})")
            if name == "rdst_pack_batch":
                jobs = (_lib.PackJob * args[1]).from_address(args[0].value)
                for i, j in enumerate(jobs):
                    w, g, be, bi, o = (self.label(p, {}) for p in (j.W, j.gamma, j.beta, j.bias, j.out))
                    self.lines.append(f"  job {i}: kind {j.kind} W {w} gamma {g} beta {be} bias {bi} out {o} N {j.N} K {j.K} s {j.s!r}")
            self.seen[name] += 1
            return _lib.ENOTSUP if self.seen[name] in self.refuse.get(name, ()) else 0
        return call

    def note(self, text):
        self.lines.append(text)

    def plan(self):
        p = ops.pack_plan_of(self.owner)
        self.note("plan: none" if p is None else
                  f"plan: misses {p.misses} arena {p.arena.numel()} specs {[list(s) for s in p.specs]}")


def traced(mp, **kw):
    rec = Recorder(**kw)
    mp.setattr(_lib, "load", lambda: rec)
    mp.setattr(ops, "_need_gpu", lambda *ts: None)
    mp.setattr(ops, "_stream", lambda: None)
    return rec


# ------------------------------------------------------------------------------------------------
# the network: embed 60, 6 heads, one RDSTB of DenseSTLayers of depth 2, growth 30, 16 x 16 patches, batch 2
# ------------------------------------------------------------------------------------------------
def make_net(mode, window=8, layers=2):
    torch.manual_seed(0)
    net = RDSTSR(img_size=16, in_chans=1, sr_scale=2, embed_dim=60, dense_layer_depths=[2], num_heads=[6], window_size=[window],
                 rdb_depths=[layers], mlp_ratio=2.0, growth_rate=30, pre_norm=True, feature_last_operation=True)
    return net.train().set_compute_dtype(mode)


def short_names(net):
    """() -> the network's (name, parameter) pairs, a DenseSTLayer's block written layer<i>.block<j>"""
    return lambda: ((n.replace("body.0.body.", "layer").replace(".body.blocks.", ".block"), p) for n, p in net.named_parameters())


def forward(net, x):
    """RDSTSR.forward (feature_last_operation) with the dense-buffer chain, which the module itself takes for device tensors
    only: the patch norm writes into the RDSTB's buffer, every DenseSTLayer appends in place and joins through a GradSink."""
    with ops.compute_scope(net.compute_code), ops.pack_scope(net):
        rows = ops.nchw_to_rows(x, net.compute_dtype)
        feat = net.head.forward_rows(net.sub_mean.forward_rows(rows))
        B, H, W, E = feat.shape
        blk = net.body[0]
        buf = blk.make_buffer(B, H * W, feat.dtype, feat.device)
        t = _norm_only(feat.view(B, H * W, E), net.patch_embed.norm, out_slot=(buf, 0))
        y = ops.into_dense(t, buf)
        for m in blk.body:
            y = m.forward_dense(y, (H, W), buf)
        t = _apply_res_connection(blk.conv, y.view(B, H, W, -1), residual=t.view(B, H, W, E), out_scale=blk.residual_scale)
        t = _norm_only(t.view(B, H * W, E), net.norm, out_scale=net.global_res_scale)
        y = _apply_res_connection(net.conv_after_body, t.view(B, H, W, E), residual=feat)
        for m in net.tail:
            y = m.forward_rows(y)
        return ops.rows_to_nchw(net.add_mean.forward_rows(y))


def batch():
    g = torch.Generator().manual_seed(3)
    return torch.rand(2, 1, 16, 16, generator=g), torch.rand(2, 1, 32, 32, generator=g)


def train_step(rec, net, bucket=None):
    """forward + L1 + backward; with a bucket the way the trainer does it (gradients written straight into the flat bucket)."""
    x, tgt = batch()
    rec.bucket = bucket
    if bucket is not None:
        bucket.detach_grads()
    rec.note("-- forward")
    y = forward(net, x)
    rec.plan()
    rec.note("-- backward")
    F.l1_loss(y, tgt).backward()
    if bucket is not None:
        bucket.gather()
    assert ops._ReduceBatch.depth == 0


def eval_forward(rec, net, what="eval forward"):
    rec.note("-- " + what)
    with torch.no_grad():
        forward(net, batch()[0])
    rec.plan()


def net_scenario(mode, window=8, layers=2, switch=None, refuse=None, steps=1, evals=0):
    def run(mp):
        if switch is not None:
            mp.setattr(ops, switch, False)
        net = make_net(mode, window, layers)
        rec = traced(mp, named=short_names(net), owner=net, refuse=refuse)
        bucket = dp.FlatGradBucket(net.parameters())
        for _ in range(steps):
            train_step(rec, net, bucket)
        plan = ops.pack_plan_of(net)      # (none where nothing is packable: exact fp32, fp32x3 without the streaming kernels)
        assert plan is None or plan.misses == 0
        for _ in range(evals):
            eval_forward(rec, net.eval())
        return rec.lines
    return run


def plan_repointed_parameter(mp):
    net = make_net("bf16", layers=1).eval()
    rec = traced(mp, named=short_names(net), owner=net)
    eval_forward(rec, net, "forward: plan recorded")
    p = net.body[0].body[0].body.blocks[0].mlp.fc1.weight
    p.data = p.data.clone()
    eval_forward(rec, net, "forward after fc1.weight.data was re-pointed: plan dropped and recorded again")
    eval_forward(rec, net, "forward: the new plan is used")
    return rec.lines


def plan_other_path(mp):
    net = make_net("bf16", layers=1).eval()
    rec = traced(mp, named=short_names(net), owner=net)
    eval_forward(rec, net, "forward: plan recorded")
    # (the attention half: flipping MLP_FUSED moves no lookup, see plan_mlp_switch_flipped)
    mp.setattr(ops, "ATTN_FUSED", False)
    eval_forward(rec, net, "forward with ATTN_FUSED off: misses, plan dropped")
    eval_forward(rec, net, "forward: recorded again")
    eval_forward(rec, net, "forward: used")
    return rec.lines


def plan_mlp_switch_flipped(mp):
    """In bf16 no Mlp shape is both fused (K7) and packable as single Linears, so this flip changes the calls but no lookup:
    the plan stays, with the K7 group unused."""
    net = make_net("bf16", layers=1).eval()
    rec = traced(mp, named=short_names(net), owner=net)
    eval_forward(rec, net, "forward: plan recorded")
    mp.setattr(ops, "MLP_FUSED", False)
    eval_forward(rec, net, "forward with MLP_FUSED off: composed Mlp, no misses, plan kept")
    return rec.lines


def plan_kept(mp):
    net = make_net("bf16", layers=1).eval()
    rec = traced(mp, named=short_names(net), owner=net)
    eval_forward(rec, net, "forward: plan recorded")
    old = ops.pack_plan_of(net)
    with ops.keep_pack_plan(net):
        mp.setattr(ops, "ATTN_FUSED", False)
        eval_forward(rec, net, "inside keep_pack_plan, ATTN_FUSED off: the plan is dropped")
        eval_forward(rec, net, "inside keep_pack_plan: another plan is recorded")
        mp.setattr(ops, "ATTN_FUSED", True)
    rec.note(f"the old plan is back: {ops.pack_plan_of(net) is old}")
    eval_forward(rec, net, "forward: the old plan is used")
    net2 = make_net("bf16", layers=1).eval()
    with ops.keep_pack_plan(net2):
        eval_forward(rec, net2, "a module without a plan inside keep_pack_plan (its arena is not labelled)")
    rec.note(f"and has none afterwards: {ops.pack_plan_of(net2) is None}")
    return rec.lines


def plan_nested_scope(mp):
    net = make_net("bf16", layers=1).eval()
    rec = traced(mp, named=short_names(net), owner=net)
    for what in ("recorded", "used"):
        with ops.pack_scope(net):
            eval_forward(rec, net, f"forward inside an outer pack_scope: the outer scope's plan is being {what}")
        rec.plan()
    return rec.lines


def grads_accumulate(mp):
    net = make_net("bf16", layers=1)
    rec = traced(mp, named=short_names(net), owner=net)
    train_step(rec, net)
    train_step(rec, net)      # no zero_grad: p.grad is defined, every destination is fresh
    return rec.lines


# ------------------------------------------------------------------------------------------------
# op level
# ------------------------------------------------------------------------------------------------
def rows(*shape, dtype=torch.bfloat16, grad=True):
    return torch.zeros(*shape, dtype=dtype).requires_grad_(grad)


def block_scenario(freeze=(), x_grad=True, outer_batch=False, switch=None, refuse=None, strided_dy=False):
    def run(mp):
        if switch is not None:
            mp.setattr(ops, switch, False)
        torch.manual_seed(0)
        blk = SwinTransformerBlock(60, (16, 16), 6, window_size=8, shift_size=4, mlp_ratio=2.0).train()
        for name, p in blk.named_parameters():
            if name in freeze:
                p.requires_grad_(False)
        rec = traced(mp, named=blk.named_parameters, refuse=refuse)
        with ops.compute_scope(ops.BF16):
            y = blk(rows(2, 256, 60, grad=x_grad), (16, 16))
        dy = torch.zeros(2, 256, 90, dtype=y.dtype)[..., 30:] if strided_dy else torch.zeros_like(y)
        rec.note("-- backward")
        if outer_batch:   # a layer's outer batch, opened by hand: the block nests in it and settles its fresh destinations
            ops._ReduceBatch.begin_layer(rec)
        y.backward(dy)
        if outer_batch:
            rec.note("-- the outer batch ends")
            ops._ReduceBatch.end(rec)
        assert ops._ReduceBatch.depth == 0
        return rec.lines
    return run


def batch_reset(mp):
    rec = traced(mp)
    ops._ReduceBatch.begin_layer(rec)
    rec.note("-- reset_backward_state() with a batch open on this thread")
    ops.reset_backward_state()
    rec.note(f"depth {ops._ReduceBatch.depth}")
    ops._ReduceBatch.begin(rec)
    ops._ReduceBatch.end(rec)
    return rec.lines


def op_ln_linear(mp):
    torch.manual_seed(0)
    lin, norm = torch.nn.Linear(60, 180), torch.nn.LayerNorm(60)
    lin2 = torch.nn.Linear(120, 60)
    lin2.weight.requires_grad_(False)      # a frozen weight with a trainable bias
    named = lambda: [("lin." + n, p) for n, p in lin.named_parameters()] + [("norm." + n, p) for n, p in norm.named_parameters()] \
        + [("lin2." + n, p) for n, p in lin2.named_parameters()]  # noqa: E731
    rec = traced(mp, named=named)
    for mode, code in (("bf16", ops.BF16), ("fp32x3", ops.F32X3), ("fp32", ops.F32)):
        dt = torch.float32 if mode != "bf16" else torch.bfloat16
        rec.note(f"-- {mode}")
        with ops.compute_scope(code):
            x = rows(2, 256, 60, dtype=dt)
            buf = ops.DenseBuffer((2, 256), 90, dt, x.device)
            ys = [ops.ln_linear(x, norm.weight, norm.bias, None, None),                                 # LayerNorm only
                  ops.ln_linear(x, norm.weight, norm.bias, lin.weight, lin.bias),
                  ops.ln_linear(x, None, None, lin.weight, None),                                       # no bias
                  ops.ln_linear(x, norm.weight, norm.bias, None, None, residual=rows(2, 256, 60, dtype=dt), out_scale=0.5),
                  ops.ln_linear(x, norm.weight, norm.bias, None, None, out_slot=(buf, 30)),
                  ops.ln_linear(rows(2, 256, 120, dtype=dt), None, None, lin2.weight, lin2.bias, in_act=ops.ACT_GELU,
                                residual=x)]
        rec.note("-- backward")
        for y in ys:
            y.backward(torch.zeros_like(y))
    return rec.lines


def op_conv_rows(mp):
    torch.manual_seed(0)
    convs = {"c60": torch.nn.Conv2d(60, 60, 3, padding=1), "up": torch.nn.Conv2d(60, 240, 3, padding=1),
             "nobias": torch.nn.Conv2d(60, 60, 3, padding=1, bias=False), "head": torch.nn.Conv2d(1, 60, 3, padding=1),
             "k1": torch.nn.Conv2d(60, 60, 1)}
    named = lambda: [(f"{k}.{n}", p) for k, c in convs.items() for n, p in c.named_parameters()]  # noqa: E731
    rec = traced(mp, named=named)
    for mode, code in (("bf16", ops.BF16), ("fp32x3", ops.F32X3), ("fp32", ops.F32)):
        dt = torch.float32 if mode != "bf16" else torch.bfloat16
        rec.note(f"-- {mode}")
        with ops.compute_scope(code):
            x = rows(2, 16, 16, 60, dtype=dt)
            buf = ops.DenseBuffer((2, 256), 120, dt, x.device)
            c = convs
            ys = [ops.conv_rows(x, c["c60"].weight, c["c60"].bias),
                  ops.conv_rows(x, c["up"].weight, c["up"].bias, shuffle=2),
                  ops.conv_rows(x, c["c60"].weight, c["c60"].bias, residual=rows(2, 16, 16, 60, dtype=dt), out_scale=0.2,
                                in_act=ops.ACT_LEAKY02),
                  ops.conv_rows(x, c["c60"].weight, c["c60"].bias, out_slot=(buf, 0)),
                  ops.conv_rows(x, c["nobias"].weight, None),
                  ops.conv_rows(rows(2, 16, 16, 1, dtype=dt, grad=False), c["head"].weight, c["head"].bias),
                  ops.conv_rows(x, c["k1"].weight, c["k1"].bias)]
        rec.note("-- backward")
        for y in ys:
            y.backward(torch.zeros_like(y))
    return rec.lines


def op_window_attention(mp):
    torch.manual_seed(0)
    at = WindowAttention(60, (8, 8), 6, attn_drop=0.1).train()
    rec = traced(mp, named=at.named_parameters)
    mask = torch.zeros(4, 64, 64)
    with ops.compute_scope(ops.BF16):
        rec.note("-- the standalone module: qkv, attention with an explicit mask and attn_drop > 0, proj")
        y1 = at(rows(8, 64, 60), mask=mask)
        rec.note("-- explicit mask, no dropout")
        y2 = ops.window_attention(rows(8, 8, 8, 180), at.relative_position_bias_table, 8, 8, 6, 8, 0, at.scale, mask=mask)
        rec.note("-- attn_drop > 0 with a seed")
        y3 = ops.window_attention(rows(2, 16, 16, 180), at.relative_position_bias_table, 16, 16, 6, 8, 4, at.scale,
                                  attn_drop=0.25, seed=torch.zeros(1, dtype=torch.int64))
    rec.note("-- backward")
    for y in (y1, y2, y3):
        y.backward(torch.zeros_like(y))
    return rec.lines


def op_layout(mp):
    rec = traced(mp)
    x = torch.zeros(2, 3, 8, 8, requires_grad=True)
    for dt in (torch.float32, torch.bfloat16):
        r = ops.nchw_to_rows(x, dt)
        y = ops.rows_to_nchw(ops.upsample_nearest2(r))
        y2 = ops.rows_to_nchw(ops.upsample_nearest2(r[..., 1:3]))     # a channel slice: strided rows, no copy
        rec.note("-- backward")
        (y.sum() + y2.sum()).backward()
    return rec.lines


SCENARIOS = {
    # the network, window 8: train step 1 records the plan, step 2 uses it, then an eval forward under no_grad
    "net fp32": net_scenario("fp32", steps=2, evals=1),
    "net fp32x3": net_scenario("fp32x3", steps=2, evals=1),
    "net bf16": net_scenario("bf16", steps=2, evals=1),
    "net bf16 window 16": net_scenario("bf16", window=16, steps=2, evals=1),
    # the module switches, one at a time
    "MLP_FUSED off": net_scenario("bf16", layers=1, switch="MLP_FUSED", steps=2),
    "ATTN_FUSED off": net_scenario("bf16", layers=1, switch="ATTN_FUSED", steps=2),
    "ATTN_LSE off, window 16": net_scenario("bf16", window=16, layers=1, switch="ATTN_LSE"),
    "X3_STREAM off, fp32x3": net_scenario("fp32x3", layers=1, switch="X3_STREAM", steps=2),
    # scripted refusals (the n-th call of a name answers ENOTSUP)
    "refused: rdst_swin_attn_fwd": net_scenario("bf16", layers=1, refuse={"rdst_swin_attn_fwd": (1, 2)}, steps=2),
    "refused: rdst_mlp_fwd, then rdst_mlp_bwd with h kept": net_scenario(
        "bf16", layers=1, refuse={"rdst_mlp_fwd": (1,), "rdst_mlp_bwd": (2,)}),
    "refused: rdst_mlp_bwd once, forward fused": net_scenario("bf16", layers=1, refuse={"rdst_mlp_bwd": (1,)}),
    "refused: rdst_mlp_bwd once on a strided gradient slice": block_scenario(strided_dy=True, refuse={"rdst_mlp_bwd": (1,)}),
    "refused: rdst_ln_linear_bwd2": net_scenario("bf16", layers=1, refuse={"rdst_ln_linear_bwd2": (1,)}),
    "refused: rdst_wattn_fwd_lse": net_scenario("bf16", window=16, layers=1, switch="ATTN_FUSED",
                                                refuse={"rdst_wattn_fwd_lse": (1,)}),
    "refused: rdst_wattn_bwd_lse": net_scenario("bf16", window=16, layers=1, switch="ATTN_FUSED",
                                                refuse={"rdst_wattn_bwd_lse": (1,)}),
    # the life cycle of a plan
    "plan: a parameter re-pointed": plan_repointed_parameter,
    "plan: another path than the recorded one": plan_other_path,
    "plan: MLP_FUSED flipped between two forwards": plan_mlp_switch_flipped,
    "plan: keep_pack_plan": plan_kept,
    "plan: nested pack_scope": plan_nested_scope,
    # gradient destinations
    "grads: second backward without zero_grad": grads_accumulate,
    "grads: block inside an open outer batch (fresh destinations settle)": block_scenario(outer_batch=True),
    "grads: frozen relative_position_bias_table": block_scenario(freeze=("attn.relative_position_bias_table",)),
    "grads: block input without requires_grad": block_scenario(x_grad=False),
    "grads: frozen Mlp weights (scratch destinations)": block_scenario(freeze=("mlp.fc1.weight", "mlp.fc2.weight")),
    "grads: frozen Mlp weights, MLP_FUSED off": block_scenario(freeze=("mlp.fc1.weight", "mlp.fc2.weight"), switch="MLP_FUSED"),
    "grads: reset_backward_state drops the open batch": batch_reset,
    # op level
    "op: ln_linear": op_ln_linear,
    "op: conv_rows": op_conv_rows,
    "op: window_attention": op_window_attention,
    "op: nchw_to_rows, rows_to_nchw, upsample_nearest2": op_layout,
}


def recorded():
    """scenario -> its records, from the table of distinct records and the per-scenario index lists"""
    t = json.load(open(TRACE))
    return {name: [t["records"][i] for i in idx] for name, idx in t["scenarios"].items()}


def write(traces):
    records = {}
    scenarios = {name: [records.setdefault(line, len(records)) for line in lines] for name, lines in traces.items()}
    with open(TRACE, "w") as f:
        f.write('{"records": [\n' + ",\n".join(json.dumps(r) for r in records) + '\n],\n"scenarios": {\n')
        f.write(",\n".join(f"{json.dumps(n)}: {json.dumps(i, separators=(',', ':'))}" for n, i in scenarios.items()) + "\n}}\n")


def run(name):
    with pytest.MonkeyPatch.context() as mp:
        try:
            return SCENARIOS[name](mp)
        finally:
            ops._ReduceBatch.abandon(Recorder())


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_ops_make_the_recorded_calls(name):
    want = recorded()[name]
    got = run(name)
    bad = [(i, w, g) for i, (w, g) in enumerate(zip(want, got)) if w != g]
    assert not bad, f"{len(bad)} of {len(want)} records differ, first at {bad[0][0]}:\n  recorded {bad[0][1]}\n  now      {bad[0][2]}"
    assert len(got) == len(want), f"{len(got)} records, {len(want)} recorded; first extra: {(got + want)[min(len(got), len(want))]}"


def test_the_trace_covers_the_entry_points_of_ops():
    """Every entry point ops.py names is reached by some scenario (a new path needs a scenario before it can hide)."""
    import re
    src = open(os.path.join(os.path.dirname(HERE), "rdst_amd", "ops.py")).read()
    named = {n for n in re.findall(r"lib\.(rdst_\w+)\(", src) if not n.endswith(QUERIES)}
    trace = recorded()
    reached = {line.split("(")[0] for lines in trace.values() for line in lines if line.startswith("rdst_")}
    assert named <= reached, sorted(named - reached)


if __name__ == "__main__" and "--record" in sys.argv:
    write({name: run(name) for name in sorted(SCENARIOS)})
    print("wrote", TRACE, os.path.getsize(TRACE), "bytes")
