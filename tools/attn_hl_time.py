"""us per call of the split-operand attention entry, qkv_attention(..., dtype=3) (conversions + attn_d64_hl_kernel), device events:
    [SDXL_LIB_PATH=<other build>] python tools/attn_hl_time.py B H N [B H N ...]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import __graft_entry__ as ge
pkg = ge.load_package()
ctx = pkg.Context(0)
a = [int(x) for x in sys.argv[1:]]
for B, H, N in zip(a[0::3], a[1::3], a[2::3]):
    q, k, v = (torch.randn(B, N, 64 * H, generator=torch.Generator().manual_seed(s)).cuda() for s in (1, 2, 3))
    best = []
    for rep in range(3):
        pkg.qkv_attention(ctx, q, k, v, None, H, 3)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            pkg.qkv_attention(ctx, q, k, v, None, H, 3)
        e1.record(); e1.synchronize()
        best.append(e0.elapsed_time(e1) / 20 * 1e3)
    print(f"dtype 3 B={B} H={H} N={N}: {min(best):8.1f} us per call (min of 3 x 20)", flush=True)
