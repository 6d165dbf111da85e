"""The per-step ControlNet add with K sources per destination (sdxl_skip_residual_add_steps_multi) on the GPU against fp64, over the segment tables
of test_gpu_controlnet_step_add.py: K = 1, 2, 3 and 4, B = 2 and 3, f32 and f16, the first and the last row of the scale table; K = 1 against
sdxl_skip_residual_add_steps bit for bit; a NaN source under scale 0 beside live ones; all scales 0; a source that ends before the unconditional
entries (cond_only); refusals that write nothing.

The bound (derived, not measured).  Per element the kernel computes, in fp32,  v_0 = dst,  v_k = fl32(s_k a_k + v_{k-1})  for the L live sources
(s_k != 0) in order, then dst = round_T(v_L).  An fma rounds once, so |v_k - (s_k a_k + v_{k-1})| <= spacing32(v_k) / 2, and every |v_k| is at most
M = |dst| + sum_k |s_k a_k| up to those roundings: |v_L - S| <= D = L spacing32(M) / 2 (1 + 2^-20) for the exact sum S.  In fp64 S is exact to 2^-53
relative per term (24-bit scale x 24-bit value fits), far below D.
  T = fp32: round_T is the last fma's own rounding, half a unit at the result:   |out - S| <= spacing32(|S| + D') / 2 (1 + 2^-20) + D',  D' = (L - 1) / L D.
  T = f16:  out = f16(v_L), half a unit of f16 at v_L, and |v_L| <= |S| + D:       |out - S| <= D + ulp16(|S| + D) / 2.
            (Not "f16(S) or its neighbour": where the sources cancel, S is small and its f16 spacing lies below D.)"""
import functools

import numpy as np
import pytest
import torch

from skip_add_ref import skip_add_expected
from test_gpu_controlnet_step_add import NAN, OP_SEGS, _bits, _spacing32
from util import seeded, ulp16

pytestmark = pytest.mark.gpu

# scales[row][k][b] for B = 3 (B = 2: the first two columns); row 1 of the device table is NaN and never named by the step index.
# first: entry 2 has every scale 0 (B = 3); sources 1 and 2 are at 0 beside live ones.  last: entry 1 has every scale 0; at B = 2 source 1 is dead.
SCALES = {"first": [[1.0, -0.37, 0.0], [0.5, 0.0, 0.0], [0.0, 2.0, 0.0], [-1.25, 0.75, 0.0]],
          "last": [[-0.37, 0.0, 1.0], [0.0, 0.0, 0.5], [0.25, 0.0, 0.0], [0.0, 0.0, -1.5]]}
ROW = {"first": 0, "last": 2}


def _table(K, B):
    t = np.full((3, K, 8), np.nan, dtype=np.float32)
    for name, r in ROW.items():
        for k in range(K):
            t[r, k, :B] = SCALES[name][k][:B]
    return torch.from_numpy(t)


@functools.lru_cache(maxsize=None)
def _data(B):
    """the destinations and four sources of every segment, fp32, drawn once per B and never written"""
    bufs = [seeded(B * r, ld, seed=100 + i) for i, (r, C, ld, off) in enumerate(OP_SEGS)]
    srcs = [[seeded(B * r, C, seed=200 + 10 * k + i) for k in range(4)] for i, (r, C, ld, off) in enumerate(OP_SEGS)]
    return bufs, srcs


def _reference(old, srcs, scales, tdt):
    """(fp64 sum of the live sources, its bound D-part: L spacing32(M) / 2 (1 + 2^-20), L)"""
    ref, mag, live = old.double(), old.double().abs(), 0
    for s, a in zip(scales, srcs):
        if s != 0.0:
            term = float(np.float32(s)) * a.double()
            ref, mag, live = ref + term, mag + term.abs(), live + 1
    return ref, live * 0.5 * _spacing32(mag) * (1 + 2.0 ** -20), live


def _check(got, old, srcs, scales, tdt, what):
    if all(s == 0.0 for s in scales):
        assert torch.equal(_bits(got), _bits(old)), f"{what}: every scale is 0 and the destination changed"
        return 0.0
    ref, D, live = _reference(old, srcs, scales, tdt)
    if tdt == torch.float32:
        before = D * (live - 1) / live      # the roundings in front of the last fma, whose own rounding is the destination's
        bound = 0.5 * _spacing32(ref.abs() + before) * (1 + 2.0 ** -20) + before
        err = (got.double() - ref).abs()
    else:
        bound = D + 0.5 * ulp16(ref.abs() + D)
        err = (got.double() - ref).abs()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite result (a source at scale 0 holds NaN and must not be read)"
    assert bool((err <= bound).all()), f"{what}: max err {err.max():.3e}"
    assert not torch.equal(got, old)
    return (got.double() - ref).abs().max().item()


@pytest.mark.parametrize("step", ["first", "last"])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("tdt", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_multi_add_op_against_fp64(pkg, ctx, tdt, B, K, step):
    """every (source, entry) at scale 0 holds NaN -- also where another source of the same chunk is live: the result is the fp64 sum of the live ones"""
    bufs32, srcs32 = _data(B)
    bufs = [b.to(tdt) for b in bufs32]
    srcs = [[s.to(tdt, copy=True) for s in ss[:K]] for ss in srcs32]      # (NaN is written into these: never into the shared draw)
    sc = [[SCALES[step][k][b] for k in range(K)] for b in range(B)]      # [b][k]
    for (r, C, ld, off), ss in zip(OP_SEGS, srcs):
        for k in range(K):
            for b in range(B):
                if sc[b][k] == 0.0:
                    ss[k][b * r:(b + 1) * r] = NAN
    table = _table(K, B).cuda()
    d = [b.cuda() for b in bufs]
    pkg.skip_residual_add_steps_multi(ctx, [(b[:, off:off + C], [x.cuda() for x in ss]) for b, ss, (_, C, _, off) in zip(d, srcs, OP_SEGS)], B, table,
                                      torch.tensor([ROW[step]], dtype=torch.int32, device="cuda"))
    worst = 0.0
    for out, buf, ss, (r, C, ld, off) in zip([b.cpu() for b in d], bufs, srcs, OP_SEGS):
        keep = torch.ones(ld, dtype=torch.bool)
        keep[off:off + C] = False
        assert torch.equal(_bits(out[:, keep]), _bits(buf[:, keep])), "columns outside the slice changed"
        for b in range(B):
            rows = slice(b * r, (b + 1) * r)
            got, old = out[rows, off:off + C], buf[rows, off:off + C]
            worst = max(worst, _check(got, old, [s[rows] for s in ss], sc[b], tdt, f"segment {(r, C, ld, off)} entry {b}"))
            # the bits: the NaN sources sit at scale 0 and enter the expected value as little as they enter the kernel
            want = torch.from_numpy(skip_add_expected(old.numpy(), [s[rows].numpy() for s in ss], sc[b], old.numpy().dtype))
            differ = int((_bits(got) != _bits(want)).sum())
            print(f"segment {(r, C, ld, off)} entry {b}: {differ} of {want.numel()} elements differ from the expected bits")
            assert differ == 0
    print(f"skip_residual_add_steps_multi K {K} B {B} {tdt} {step} row: max |out - fp64| {worst:.3e}")


@pytest.mark.parametrize("tdt", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_multi_add_op_one_source_is_the_step_add_bit_for_bit(pkg, ctx, tdt):
    B = 3
    bufs32, srcs32 = _data(B)
    bufs, srcs = [b.to(tdt) for b in bufs32], [ss[0].to(tdt) for ss in srcs32]
    table = torch.tensor([[1.0, -0.37, 0.0] + [NAN] * 5, [0.3, 0.0, -2.0] + [NAN] * 5], dtype=torch.float32).cuda()
    for step in (0, 1):
        one, many = [b.cuda() for b in bufs], [b.cuda() for b in bufs]
        s = [x.cuda() for x in srcs]
        pkg.skip_residual_add_steps(ctx, [(b[:, off:off + C], x) for b, x, (_, C, _, off) in zip(one, s, OP_SEGS)], B, table, step)
        pkg.skip_residual_add_steps_multi(ctx, [(b[:, off:off + C], [x]) for b, x, (_, C, _, off) in zip(many, s, OP_SEGS)], B, table.view(2, 1, 8), step)
        for a, b, buf in zip(one, many, bufs):
            assert torch.equal(_bits(a.cpu()), _bits(b.cpu()))
            assert not torch.equal(_bits(a.cpu()), _bits(buf))


@pytest.mark.parametrize("K", [1, 2, 4])
def test_multi_add_op_all_scales_zero_writes_nothing(pkg, ctx, K):
    r, C = 37, 64
    buf = seeded(2 * r, C, seed=3).half()
    srcs = [torch.full((2 * r, C), NAN, dtype=torch.float16).cuda() for _ in range(K)]
    table = torch.zeros(2, K, 8)
    table[1] = NAN
    d = buf.cuda()
    pkg.skip_residual_add_steps_multi(ctx, [(d, srcs)], 2, table.cuda(), 0)
    assert torch.equal(_bits(d.cpu()), _bits(buf))


@pytest.mark.parametrize("tdt", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_multi_add_op_short_source_stands_for_cond_only(pkg, ctx, tdt):
    """a net that ran on the conditional entries alone holds the first rows / B * n rows; the unconditional entries are at scale 0 in its rows of the
    table and the kernel does not look behind its end.  The short source lies inside a larger allocation that holds NaN in front of it and
    behind it -- behind it for as many rows as a full-length source would have, so a read there, multiplied by 0 or not, makes the result NaN --,
    the destination is a column slice of a wider buffer, and the whole allocation is compared bit for bit afterwards."""
    n, r, C, ld, off = 2, 37, 64, 192, 64
    B = 2 * n
    buf = seeded(B * r, ld, seed=11).to(tdt)
    full = seeded(B * r, C, seed=12).to(tdt)
    pool = torch.full((5 + B * r, C), NAN, dtype=tdt)
    pool[5:5 + n * r] = seeded(n * r, C, seed=13).to(tdt)
    pool_d = pool.cuda()
    short = pool_d[5:5 + n * r]
    assert short.data_ptr() % 16 == 0
    t = np.zeros((2, 2, 8), dtype=np.float32)
    t[0, 0, :B] = [1.0, -0.37, 0.5, 0.25]      # net 0: all four entries
    t[0, 1, :n] = [0.75, -1.5]                 # net 1: cond_only
    table = torch.from_numpy(t).cuda()
    d = buf.cuda()
    pkg.skip_residual_add_steps_multi(ctx, [(d[:, off:off + C], [full.cuda(), short])], B, table, 0)
    out = d.cpu()
    keep = torch.ones(ld, dtype=torch.bool)
    keep[off:off + C] = False
    assert torch.equal(_bits(out[:, keep]), _bits(buf[:, keep])), "columns outside the slice changed"
    assert torch.equal(_bits(pool_d.cpu()), _bits(pool)), "the allocation around the short source changed"
    for b in range(B):
        rows = slice(b * r, (b + 1) * r)
        srcs = [full[rows], pool[5:5 + n * r][rows] if b < n else torch.full((r, C), NAN, dtype=tdt)]
        _check(out[rows, off:off + C], buf[rows, off:off + C], srcs, [float(t[0, 0, b]), float(t[0, 1, b])], tdt, f"entry {b}")
    # the wrapper refuses a short source whose missing entries are live in the named row
    t[1, 1, :B] = 1.0
    d = buf.cuda()
    with pytest.raises(pkg.InvalidArgument, match="short source"):
        pkg.skip_residual_add_steps_multi(ctx, [(d[:, off:off + C], [full.cuda(), short])], B, torch.from_numpy(t).cuda(), 1)
    assert torch.equal(_bits(d.cpu()), _bits(buf))


def test_multi_add_op_refusals_write_nothing(pkg, ctx):
    import ctypes
    buf, src = seeded(6, 64, seed=1), seeded(6, 64, seed=2)
    table = torch.ones(2, 2, 8, device="cuda")
    two = lambda: [src.cuda(), src.cuda()]
    for B, word in ((4, "multiple of B"), (0, "1..8"), (9, "1..8")):
        d = buf.cuda()
        with pytest.raises(pkg.InvalidArgument, match=word):
            pkg.skip_residual_add_steps_multi(ctx, [(d, two())], B, table, 0)
        assert torch.equal(d.cpu(), buf)
    d = buf.cuda()
    flat = torch.zeros(6 * 64 + 4, device="cuda")
    with pytest.raises(pkg.InvalidArgument, match="aligned"):      # the second source off a 16-byte boundary
        pkg.skip_residual_add_steps_multi(ctx, [(d, [src.cuda(), flat[1:1 + 6 * 64].view(6, 64)])], 2, table, 0)
    with pytest.raises(pkg.InvalidArgument):      # the destination off a 16-byte boundary
        pkg.skip_residual_add_steps_multi(ctx, [(d[:, 1:9], [src[:, :8].contiguous().cuda()] * 2)], 2, table, 0)
    with pytest.raises(pkg.InvalidArgument, match="step_idx"):
        pkg.skip_residual_add_steps_multi(ctx, [(d, two())], 2, table, 2)
    with pytest.raises(pkg.InvalidArgument, match="scales"):      # a table for another K
        pkg.skip_residual_add_steps_multi(ctx, [(d, two())], 2, table[:, :1].contiguous(), 0)
    with pytest.raises(pkg.InvalidArgument, match="1..4"):
        pkg.skip_residual_add_steps_multi(ctx, [(d, [src.cuda()] * 5)], 2, torch.ones(2, 5, 8, device="cuda"), 0)
    # K outside 1 .. SDXL_MAX_CONTROLS and a null source at the C entry itself
    s = src.cuda()
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    dst, ld = (ctypes.c_void_p * 1)(d.data_ptr()), (ctypes.c_int64 * 1)(64)
    rows, cols = (ctypes.c_int64 * 1)(6), (ctypes.c_int32 * 1)(64)
    big = torch.ones(2, 8, 8, device="cuda")
    for K, ptrs in ((0, [s.data_ptr()] * 5), (5, [s.data_ptr()] * 5), (2, [s.data_ptr(), None])):
        srcs = (ctypes.c_void_p * 5)(*ptrs)
        rc = pkg.lib().sdxl_skip_residual_add_steps_multi(ctx.h, None, 1, dst, ld, srcs, K, rows, cols, 2, ctypes.c_void_p(big.data_ptr()),
                                                          ctypes.c_void_p(idx.data_ptr()), pkg.DTYPE_F32)
        assert rc != 0, f"K {K} was not refused"
    torch.cuda.synchronize()
    assert torch.equal(d.cpu(), buf)
