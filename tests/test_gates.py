"""Why the fp32x3 tests gate tile by tile (tests/util.py: local_rel), replayed on CPU tensors.

A kernel tile that loses the lo term of its split-bf16 operands computes at bf16 precision: ~1e-3 relative where the rest of
the tensor sits at the fp32x3 level (3.5e-6 per op, README).  One relative L2 over a whole 70003 x 360 or 131072 x 360 tensor
averages that tile away and the old gate (<= 3e-5) passes it; the worst 32 x 32 tile of local_rel is more than 100x above
the median and fails any tile gate <= 3e-4 (the cap the fp32x3 op tests use)."""
import torch

from util import local_rel

NOISE = 3.5e-6       # the fp32x3 per-op relative error
OLD_GATE = 3e-5      # the global relative-L2 gate of the fp32x3 op tests
TILE_CAP = 3e-4      # the largest tile gate any fp32x3 test may use


def _tensor(M, N, seed):
    g = torch.Generator().manual_seed(seed)
    want = torch.randn(M, N, generator=g, dtype=torch.float64)
    got = want + NOISE * torch.randn(M, N, generator=g, dtype=torch.float64)
    return got, want


def _global(got, want):
    return ((got - want).norm() / want.norm()).item()


def _bf16(t):
    return t.to(torch.bfloat16).to(torch.float64)


def test_clean_tensor_passes_both_gates():
    got, want = _tensor(70003, 360, 1)
    worst, med, _ = local_rel(got, want, {0: 32, 1: 32})
    assert _global(got, want) <= OLD_GATE
    assert worst <= 2 * NOISE and 0.5 * NOISE <= med <= 1.5 * NOISE


def test_bf16_tail_rows_pass_the_old_gate_and_fail_the_tile_gate():
    """The 3 rows of the ragged last tile at M = 70003 rounded to bf16: padded, not dropped, and caught."""
    got, want = _tensor(70003, 360, 2)
    got[-3:] = _bf16(want[-3:])
    g = _global(got, want)
    worst, med, idx = local_rel(got, want, {0: 32, 1: 32})
    print(f"\n3 bf16 tail rows: global {g:.2e}  tile worst {worst:.2e} median {med:.2e} at {idx}")
    assert g <= OLD_GATE                               # the old gate passes the bad tile ...
    assert worst > TILE_CAP and worst > 100 * med      # ... the tile gate does not
    assert idx[0] == 70003 // 32                       # and names the ragged tile


def test_one_bf16_tile_passes_the_old_gate_at_bench_size_and_fails_the_tile_gate():
    """One whole 32-row tile at bf16 precision at the bench's M = 131072."""
    got, want = _tensor(131072, 360, 3)
    got[32 * 1000:32 * 1001] = _bf16(want[32 * 1000:32 * 1001])
    g = _global(got, want)
    worst, med, idx = local_rel(got, want, {0: 32, 1: 32})
    rows, _, ridx = local_rel(got, want, {0: 32})
    print(f"\none bf16 tile: global {g:.2e}  tile worst {worst:.2e} median {med:.2e} at {idx}")
    assert g <= OLD_GATE
    assert worst > TILE_CAP and worst > 100 * med and idx[0] == 1000
    assert rows > TILE_CAP and ridx == (1000,)


def test_local_rel_blocks():
    """Block layout: named dims cut into blocks (ragged ones padded), the others whole; the index is in block coordinates."""
    want = torch.ones(5, 7, 3, dtype=torch.float64)
    got = want.clone()
    got[4, 6, 0] += 0.5                                   # in the ragged corner block of a 2 x 4 tiling of dims 0 and 1
    worst, med, idx = local_rel(got, want, {0: 2, 1: 4})
    assert idx == (2, 1)
    assert abs(worst - 0.5 / 9 ** 0.5) < 1e-12           # its real part: row 4 x columns 4..6 x 3 = 9 elements
    assert med == 0.0
    worst, _, idx = local_rel(got, want, {2: 1})          # one block per index of the last dim
    assert idx == (0,) and abs(worst - 0.5 / 35 ** 0.5) < 1e-12
    worst, _, idx = local_rel(got.float(), want, {-1: 3})  # negative dims; one block for the whole tensor here
    assert idx == (0,) and abs(worst - 0.5 / 105 ** 0.5) < 1e-7
