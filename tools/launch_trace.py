#!/usr/bin/env python3
"""Which kernels do the launchers pick?  Every C entry point with a choice of kernels behind it is called directly at the small
shapes that decide the choice: window attention forward and backward (ws 4 / 8 / 16, heads 6 / 3, C 48 / 60 / 90 / 120, dense
rows, strided rows, a base pointer off by 4 bytes, an explicit mask, bf16 / fp32 / fp32x3; 2 to 4 windows, so fewer slab rows
than the 256 of a full grid), the fused Mlp forward (with and without the packed-weight workspace) and backward at C 48 / 60 /
120, the bf16 Linear backward at (60, 180), (120, 30), (48, 48) with and without LayerNorm, the fp32 / fp32x3 Linear backward
at (60, 180) and (120, 360) behind a LayerNorm (the latter in two half launches) and (60, 60) plain, at 64 and 4096 tokens, and
the conv backward in the three modes at 1 x 32 x 32: the three register-stationary shapes, a generic 100 -> 130 conv and the
one-channel tail and head convs.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/launch_trace.py run     # one line per call on stdout
    python tools/launch_trace.py summarize DIR/**/*_kernel_trace.csv > LIST                     # name, grid, workgroup, LDS

Run both once per library (RDST_HIP_LIB=<other build>) and compare the two lists line for line.  tools/op_hashes.py runs the
same calls for their values."""
import csv
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DT = {"bf16": 1, "fp32": 0, "fp32x3": 2}   # _lib.BF16 / F32 / F32X3


def _rows(torch, n, width, ld, dtype, seed, off_bytes=0, fill=True):
    """(tensor that owns the memory, address of row 0): n rows of `width` elements, `ld` apart, `off_bytes` into the buffer"""
    es = 2 if dtype == torch.bfloat16 else 4
    pad = off_bytes // es
    host = torch.zeros(n * ld + pad, dtype=torch.float32)
    if fill:
        v = torch.randn((n, width), generator=torch.Generator().manual_seed(seed))
        host[pad:].view(n, ld)[:, :width] = v
    t = host.to(dtype).cuda()
    return t, t.data_ptr() + off_bytes


def _par(torch, shape, seed, s=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * s).cuda()


def wattn_cases():
    for dt, ws, heads, C in itertools.product(DT, (4, 8, 16), (6, 3), (48, 60, 90, 120)):
        for layout in ("dense", "strided", "off4"):
            yield dt, ws, heads, C, layout, ws // 2, False
    for dt, ws in itertools.product(DT, (8, 16)):   # no shift; an explicit mask (only the scalar kernels take one)
        yield dt, ws, 6, 60, "dense", 0, False
        yield dt, ws, 6, 60, "dense", ws // 2, True


def wattn(torch, lib, dt, ws, heads, C, layout, shift, mask):
    """-> (rc forward, rc backward, {name: tensor})"""
    B, H, W = 1, 2 * ws, (4 if ws == 4 else 2) * ws   # 4 / 2 / 2 windows
    n, N = B * H * W, ws * ws
    tdt = torch.bfloat16 if dt == "bf16" else torch.float32
    pad, off = (8 if layout == "strided" else 0), (4 if layout == "off4" else 0)
    ld3, ld1 = 3 * C + pad, C + pad
    qkv, pq = _rows(torch, n, 3 * C, ld3, tdt, 1, off)
    dout, pd = _rows(torch, n, C, ld1, tdt, 2, off)
    out, po = _rows(torch, n, C, ld1, tdt, 0, off, fill=False)
    dqkv, pdq = _rows(torch, n, 3 * C, ld3, tdt, 0, off, fill=False)
    table = _par(torch, ((2 * ws - 1) ** 2, heads), 3, 0.5)
    dtable = torch.zeros_like(table)
    nw = (H // ws) * (W // ws)
    m = _par(torch, (nw, N, N), 4) if mask else None
    nb = lib.rdst_wattn_bwd_workspace(B, H, W, C, heads, ws)
    wsp = torch.empty(nb, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    scale = (C // heads) ** -0.5
    mp = m.data_ptr() if mask else None
    rf = lib.rdst_wattn_fwd(pq, ld3, table.data_ptr(), mp, nw if mask else 0, po, ld1, B, H, W, C, heads, ws, shift, scale, DT[dt], st)
    rb = lib.rdst_wattn_bwd(pq, ld3, table.data_ptr(), mp, nw if mask else 0, pd, ld1, pdq, ld3, dtable.data_ptr(), wsp.data_ptr(), nb,
                            B, H, W, C, heads, ws, shift, scale, DT[dt], st)
    torch.cuda.synchronize()
    return rf, rb, {"out": out, "dqkv": dqkv, "dtable": dtable}


def mlp(torch, lib, C, packed, M=160):
    """bf16 fused Mlp: -> (rc forward, rc backward, tensors)"""
    hid = 2 * C
    x, px = _rows(torch, M, C, C, torch.bfloat16, 1)
    gy, pg = _rows(torch, M, C, C, torch.bfloat16, 2)
    y, dx = torch.zeros_like(x), torch.zeros_like(x)
    lw, lb = 1 + _par(torch, (C,), 3, 0.1), _par(torch, (C,), 4, 0.1)
    w1, b1 = _par(torch, (hid, C), 5, C ** -0.5), _par(torch, (hid,), 6, 0.1)
    w2, b2 = _par(torch, (C, hid), 7, hid ** -0.5), _par(torch, (C,), 8, 0.1)
    stats = torch.zeros((M, 2), device="cuda")
    g = [torch.zeros_like(t) for t in (w1, b1, w2, b2, lw, lb)]
    nf = lib.rdst_mlp_fwd_workspace(C, hid) if packed else 0
    wf = torch.empty(nf + 16, dtype=torch.uint8, device="cuda")
    nb = lib.rdst_mlp_bwd_workspace(M, C, hid)
    wb = torch.empty(nb, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    rf = lib.rdst_mlp_fwd(px, C, lw.data_ptr(), lb.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), y.data_ptr(), C,
                          stats.data_ptr(), wf.data_ptr() if packed else None, nf, M, C, hid, 1, st)
    rb = lib.rdst_mlp_bwd(px, C, lw.data_ptr(), lb.data_ptr(), stats.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), pg, C,
                          dx.data_ptr(), C, *[t.data_ptr() for t in g], wb.data_ptr(), nb, M, C, hid, 1, st)
    torch.cuda.synchronize()
    return rf, rb, dict(zip(("y", "stats", "dx", "dW1", "db1", "dW2", "db2", "dg", "dbeta"), [y, stats, dx, *g]))


def linear_bwd(torch, lib, K, N, ln, M=160, dt="bf16"):
    """Linear backward (one pass where the shape allows): -> (rc, tensors)"""
    tdt = torch.bfloat16 if dt == "bf16" else torch.float32
    x, px = _rows(torch, M, K, K, tdt, 1)
    gy, pg = _rows(torch, M, N, N, tdt, 2)
    dx = torch.zeros_like(x)
    w = _par(torch, (N, K), 3, K ** -0.5)
    lw, lb = 1 + _par(torch, (K,), 4, 0.1), _par(torch, (K,), 5, 0.1)
    xf = x.float().view(M, K)
    stats = torch.stack([xf.mean(-1), (xf.var(-1, unbiased=False) + 1e-5).rsqrt()], dim=1).contiguous()
    dw, db, dlw, dlb = torch.zeros_like(w), torch.zeros(N, device="cuda"), torch.zeros_like(lw), torch.zeros_like(lb)
    nb = lib.rdst_ln_linear_bwd_workspace(M, K, N)
    wsp = torch.empty(nb, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = lib.rdst_ln_linear_bwd(px, K, lw.data_ptr() if ln else None, lb.data_ptr() if ln else None, stats.data_ptr() if ln else None, 0,
                                w.data_ptr(), pg, N, dx.data_ptr(), K, None, 0, dw.data_ptr(), db.data_ptr(),
                                dlw.data_ptr() if ln else None, dlb.data_ptr() if ln else None, wsp.data_ptr(), nb, M, K, N, 1.0, DT[dt],
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, {"dx": dx, "dW": dw, "db": db, **({"dg": dlw, "dbeta": dlb} if ln else {})}


CONVS = ((150, 60, 3, 1), (60, 60, 3, 1), (60, 240, 3, 2), (100, 130, 3, 1), (60, 1, 3, 1), (1, 60, 3, 1))   # Cin, Cout, ks, shuffle


def conv_bwd(torch, lib, dt, Cin, Cout, ks, r, B=1, H=32, W=32):
    """conv backward, every gradient (the head conv: no data gradient): -> (rc, tensors)"""
    tdt = torch.bfloat16 if dt == "bf16" else torch.float32
    n, cy = B * H * W, Cout // (r * r)
    x, px = _rows(torch, n, Cin, Cin, tdt, 1)
    gy, pg = _rows(torch, n * r * r, cy, cy, tdt, 2)
    dx = torch.zeros_like(x)
    w = _par(torch, (Cout, Cin, ks, ks), 3, (Cin * ks * ks) ** -0.5)
    dw, db = torch.zeros_like(w), torch.zeros(Cout, device="cuda")
    nb = lib.rdst_conv_bwd_workspace(B, H, W, Cin, Cout, ks)
    wsp = torch.empty(nb, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = lib.rdst_conv_bwd(px, Cin, 0, w.data_ptr(), pg, cy, dx.data_ptr() if Cin > 1 else None, Cin, None, 0, dw.data_ptr(), db.data_ptr(),
                           wsp.data_ptr(), nb, B, H, W, Cin, Cout, ks, 1.0, r, DT[dt], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, {"dx": dx, "dW": dw, "db": db}


def calls(torch, lib):
    """(label, return codes, tensors) of every call of the list"""
    for c in wattn_cases():
        rf, rb, t = wattn(torch, lib, *c)
        yield "wattn %s ws%d h%d C%d %s shift%d%s" % (*c[:6], " mask" if c[6] else ""), (rf, rb), t
    for C, packed in itertools.product((48, 60, 120), (False, True)):
        rf, rb, t = mlp(torch, lib, C, packed)
        yield "mlp C%d%s" % (C, " packed" if packed else ""), (rf, rb), t
    for (K, N), ln in itertools.product(((60, 180), (120, 30), (48, 48)), (True, False)):
        rc, t = linear_bwd(torch, lib, K, N, ln)
        yield "linear_bwd %d->%d%s" % (K, N, " ln" if ln else ""), (rc,), t
    for dt, (K, N, ln), M in itertools.product(("fp32", "fp32x3"), ((60, 180, True), (120, 360, True), (60, 60, False)), (64, 4096)):
        rc, t = linear_bwd(torch, lib, K, N, ln, M, dt)
        yield "linear_bwd %s %d->%d%s M%d" % (dt, K, N, " ln" if ln else "", M), (rc,), t
    for dt, c in itertools.product(DT, CONVS):
        rc, t = conv_bwd(torch, lib, dt, *c)
        yield "conv_bwd %s %d->%d k%d r%d" % (dt, *c), (rc,), t


def summarize(paths):
    rows = []
    for p in paths:
        rows += list(csv.DictReader(open(p)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    for r in rows:
        if "at::native" in r["Kernel_Name"]:   # (torch's own fills and reductions while the inputs are made)
            continue
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        print(f"{name} grid={r['Grid_Size_X']} wg={r['Workgroup_Size_X']} lds={r['LDS_Block_Size']}")


if __name__ == "__main__":
    if sys.argv[1:2] == ["summarize"]:
        summarize(sys.argv[2:])
    elif sys.argv[1:2] == ["run"]:
        import torch
        from rdst_amd import _lib
        for label, rcs, _ in calls(torch, _lib.load()):
            print(label, *rcs, flush=True)
    else:
        sys.exit(__doc__)
