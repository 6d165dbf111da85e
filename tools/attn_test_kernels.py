"""Which head-dim-64 attention kernel each qkv_attention test case of tests/test_gpu_ops.py and tests/test_gpu_f16_kernels.py launches, as
sdxl_debug_attn_select answers on the CPU (no GPU needed).  The case lists mirror the tests' parametrisations (B, heads, Nq, Nk, dtype, masked,
forced attn_variant); the single-op entry hands unmasked f16 calls the cross-workgroup workspace (capi_ops.hip: give_xsplit_ws), dtype 3 goes to
attn_d64_hl_kernel without a selection, head dim 512 to attn_hd_kernel.
    python tools/attn_test_kernels.py"""
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge
import select_cases as sc

OPS, F16K = "test_gpu_ops.py::", "test_gpu_f16_kernels.py::"
SHAPES_V = [(2, 2, 256, 256), (2, 10, 300, 77), (1, 20, 1024, 1024), (1, 1, 130, 200), (2, 1, 64, 1), (2, 2, 100, 128), (1, 1, 33, 192), (2, 5, 300, 320),
            (3, 10, 1000, 192)]
CASES = []      # (test, B, H, Nq, Nk, dtype, masked, variant)
for dt in (0, 1):
    CASES += [(OPS + "test_qkv_attention", B, H, Nq, Nk, dt, m, 0) for B, H, Nq, Nk, m in
              [(1, 1, 64, 64, 0), (2, 2, 256, 256, 0), (2, 10, 300, 77, 0), (1, 2, 77, 77, 1), (1, 20, 1024, 1024, 0)]]
CASES += [(OPS + "test_qkv_attention_online_softmax_rescale", 1, 1, 320, 320, dt, 0, v) for dt, v in [(0, 0), (1, 0), (1, 1), (1, 2), (1, 6), (1, 7), (1, 8)]]
CASES += [(OPS + "test_qkv_attention_f16_variants", B, H, Nq, Nk, 1, 0, v) for v in (1, 2, 6, 7, 8) for B, H, Nq, Nk in SHAPES_V]
for v, H, N, B in [(7, 10, 384, 3), (8, 20, 320, 3), (0, 10, 3328, 2), (0, 20, 256, 3)]:
    CASES += [(OPS + "test_qkv_attention_mixed_block_sizes_are_their_bodies", b, H, N, N, 1, 0, x) for b in (B, 1) for x in sorted({v, 6, 2 if v == 7 else 6})]
CASES += [(OPS + "test_qkv_attention_key_halves_across_workgroups", b, H, N, N, 1, 0, 0) for B, H, N in [(2, 20, 1024), (1, 20, 1024), (3, 10, 384), (1, 5, 128), (2, 5, 2048)]
          for b in sorted({B, 1})]
CASES += [(F16K + "test_attention_single_key_returns_f16_v", 2, 10, 320, 1, 1, 0, v) for v in (0, 6, 7, 8)]
CASES += [(F16K + "test_self_attention_d64", B, H, N, N, 1, 0, 0) for B in (2, 1) for N, H in [(4096, 10), (1024, 20), (4096, 12), (1024, 24), (256, 24)]]
CASES += [(F16K + "test_self_attention_d64_forced_variants", B, H, N, N, 1, 0, v) for v, B, N, H in [(6, 2, 1024, 20), (7, 2, 4096, 10), (8, 2, 1024, 20), (6, 1, 4096, 12)]]
CASES += [(F16K + "test_self_attention_d64_late_max_jumps", 1, 10, 4096, 4096, 1, 0, v) for v in (0, 2, 6)]
CASES += [(F16K + "test_cross_attention_77_keys", B, C // 64, Nq, 77, 1, 0, 0) for B, Nq, C in [(2, 1024, 1280), (2, 4096, 640), (2, 4096, 768), (2, 1024, 1536)]]
CASES += [(F16K + "test_masked_attention_clip_causal", 2, 12, 77, 77, 1, 1, 0)]


def name(c):
    if c.kernel == 4:
        bodies = {0: "attn_d64_body<1> + <2>", 1: "attn_d64_body<2> + <4>", 2: "attn_d64_body<2> + <2, XH>"}[c.mix]
        return f"attn_d64_mix_kernel<{c.mix}> ({bodies}; {c.big_heads} heads in large blocks)", f"MIX {c.mix}"
    if c.kernel == 3:
        return "attn_d64_ks_kernel<2, 0> (attn_d64_body<2>)", "KS"
    if c.kernel == 2:
        return f"attn_d64_v2_kernel<{c.ns}> (attn_d64_body<1>)", "V2"
    if c.kernel == 1:
        return "attn_d64_f16_kernel", "F16"
    return ("attn_d64_kernel<_Float16>", "GENERIC f16") if c.elem == sc.F16 else ("attn_d64_kernel<float>", "GENERIC f32")


lib = ge.load_package().lib()
seen = collections.Counter()
for test, B, H, Nq, Nk, dt, masked, v in CASES:
    case = sc.AttnCase(B=B, H=H, Nq=Nq, Nk=Nk, dt=sc.F16 if dt == 1 else sc.F32, present=(sc.MASK if masked else 0) | (sc.XSPLIT_WS if dt == 1 and not masked else 0), misaligned=0)
    out = sc.AttnChoice()
    assert lib.sdxl_debug_attn_select(sc.ctypes.byref(case), sc.ctypes.byref(sc.Knobs(**dict(sc.DEFAULT_KNOBS, attn_variant=v))), sc.ctypes.byref(out)) == 0
    full, short = name(out)
    seen[short] += 1
    print(f"{test:75s} B={B} H={H:2d} Nq={Nq:4d} Nk={Nk:4d} dtype={dt} mask={masked} variant={v}: {full}, grid {out.grid_x} x {out.grid_y}")
print("kernels reached: " + ", ".join(f"{k} ({n})" for k, n in sorted(seen.items())))
