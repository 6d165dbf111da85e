"""The GEMM / attention kernel selection (csrc/select.cpp) on the CPU: the table of what the launchers chose before the selection
had a home of its own, the batch-independence of every rule that changes output bits, the host code under sanitizers, and what the
refiner's block cases (tests/unet_block_ref.py) are there to reach."""
import collections
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import select_cases as sc
import unet_block_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def built(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return pkg


@pytest.fixture(scope="module")
def table():
    """the recorded table: distinct result rows + one index per case"""
    t = np.load(os.path.join(GOLDEN, "select_table.npz"))
    return {"igemm": t["igemm_rows"][t["igemm_index"]], "attn": t["attn_rows"][t["attn_index"]],
            "errors": json.load(open(os.path.join(GOLDEN, "select_table_errors.json")))}


@pytest.fixture(scope="module")
def selected(built):
    """every case through the library's two debug entries, once"""
    lib = ctypes.CDLL(built.LIB_PATH)
    return {which: sc.run(lib, which) for which in ("igemm", "attn")}


@pytest.mark.parametrize("which", ["igemm", "attn"])
def test_selection_reproduces_recorded_table(selected, table, which):
    """every case: the same kernel instantiation, grid, LDS bytes, split-K count and predicate answers -- or the same refusal text"""
    rows, errors = selected[which]
    want = table[which]
    assert errors == table["errors"][which]
    assert rows.shape == want.shape
    bad = np.nonzero((rows != want).any(axis=1))[0]
    assert bad.size == 0, (bad.size, bad[:5].tolist(), rows[bad[0]].tolist(), want[bad[0]].tolist())


def _batch_dependent(cases, rows, batch_key, signature):
    groups = collections.defaultdict(set)
    for (case, knobs), row in zip(cases, rows):
        if sc.is_default(knobs) and case[batch_key] > 0:
            groups[tuple(v for k, v in case.items() if k != batch_key)].add(signature(row))
    return len(groups), [k for k, v in groups.items() if len(v) > 1]


@pytest.mark.parametrize("source", ["library", "table"])
def test_bit_changing_rules_do_not_depend_on_the_batch(selected, table, source):
    """default knobs, B = 1 ... 8: weights-in-registers or not, the split-K count, gn_part acceptance; attention kernel and mix level --
    in what the library selects now, and in the table recorded before (no case had to be left out)"""
    igemm, attn = (selected["igemm"][0], selected["attn"][0]) if source == "library" else (table["igemm"], table["attn"])
    f = sc.IGEMM_CHOICE_FIELDS.index
    n, bad = _batch_dependent(sc.igemm_cases(), igemm, "batch", lambda r: (int(r[-1] != 0), int(r[f("family")] == 4), int(r[f("splitk")]), int(r[f("gn_part_ok")]),
                                                                         int(r[f("wreg_selected")]), int(r[f("wreg_xattn_selected")])))
    assert n > 20000 and not bad, bad[:5]
    n, bad = _batch_dependent(sc.attn_cases(), attn, "B", lambda r: (int(r[0]), int(r[1])))
    assert n >= 400 and not bad, bad[:5]


def test_selection_under_sanitizers(tmp_path, table):
    """select.cpp + a stand-alone driver built with AddressSanitizer and UBSan, the whole case list through it"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    files = []
    for which, Case, gen in (("igemm", sc.IgemmCase, sc.igemm_cases), ("attn", sc.AttnCase, sc.attn_cases)):
        files.append(str(tmp_path / (which + ".bin")))
        with open(files[-1], "wb") as fh:
            for case, knobs in gen():
                fh.write(bytes(Case(**case)) + bytes(sc.Knobs(**knobs)))
    exe = str(tmp_path / "select_driver")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                    os.path.join(ROOT, "tests", "select_driver.cpp"), os.path.join(ROOT, "stable-diffusion-xl-burn_amd", "csrc", "select.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe] + files, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    (ig, ig_refused, _), (at, at_refused, _) = (tuple(map(int, line.split())) for line in r.stdout.splitlines())
    assert (ig + ig_refused, ig_refused) == (len(table["igemm"]), int((table["igemm"][:, -1] != 0).sum()))
    assert (at + at_refused, at_refused) == (len(table["attn"]), int((table["attn"][:, -1] != 0).sum()))


# ------------------------------------------------------------------------------------------------------------------ the refiner's block cases
# What tests/unet_block_ref.py says its refiner cases reach, asked of the selection itself (default knobs, the CFG pair).  The expected values are
# the rules of csrc/select.cpp applied by hand, not its answers:
#   igemm_splitk_slices: a plain epilogue with a workspace, N <= 1536, Kpad / 64 >= 160 (K >= 10240) and at most 1024 rows per entry -> 8 slices where
#     an entry has at most 256 rows, else 3; everything else 1;
#   igemm_gn_part_ok on a split-K launch: whole 256-row tiles inside one entry (rows % 256 == 0), f16 -> f16 or split-operand -> fp32.
# (case, convolution of its ResBlock / the entry's own, slices, statistics from the epilogue)
RF_CONVS = (
    ("rf_res_384", "conv_out", 1, None),                  # K = 3456
    ("rf_rest_768_skip", "conv_out", 1, None),            # K = 6912
    ("rf_rest_1536_skip", "conv_out", 3, True),           # K = 13824, 1024 rows
    ("rf_rest_1536", "conv_out", 8, True),                # 256 rows
    ("rf_rest_1536_bucket", "conv_out", 3, False),        # 1008 rows
    ("rf_down_1536", "down", 8, False),                   # 64 rows out
    ("rf_res_1536_deep", "conv_in", 8, True),
    ("rf_res_1536_deep", "conv_out", 8, True),
    ("rf_res_1536_deep_bucket", "conv_in", 8, False),     # 252 rows
    ("rf_res_1536_deep_bucket", "conv_out", 8, False),
    ("rf_middle_1536_bucket", "conv_out", 8, False),
    ("rf_out_3072", "conv_in", 8, False),                 # K = 27648, 64 rows
    ("rf_out_3072", "conv_out", 8, False),
    ("rf_out_3072_up", "conv_in", 8, True),
    ("rf_out_3072_up_bucket", "conv_in", 8, False),
    ("rf_out_3072_up_bucket", "conv_out", 8, False),
    ("rf_out_2304", "conv_in", 8, True),                  # K = 20736, N = 768
    ("rf_out_2304", "conv_out", 1, None),                 # K = 6912
    ("rf_out_1152_res", "conv_in", 8, True),              # K = 10368: 162 k-tiles, N = 384
    ("rf_out_1152_res", "conv_out", 1, None),             # K = 3456
    ("rf_head", "conv_out", 1, None),                     # N = 4
)
# attn_select, f16, no mask: the key-split kernel (AT_KS = 3) where the keys are whole 64-key tiles and 128-query blocks x heads < 256, the mixed-block
# kernel (AT_MIX = 4) only for H % 5 == 0, else 128-query blocks (AT_V2 = 2).  256 queries x 12 / 24 heads: 2 x 24 blocks, 1024 x 24: 8 x 24 = 192 -> key-split;
# 252 and 1008 keys are no multiple of 64 -> AT_V2
RF_ATTENTION = (("rf_rest_768_skip", 12, 256, 3), ("rf_out_2304", 12, 256, 3), ("rf_rest_1536", 24, 256, 3), ("rf_rest_1536_skip", 24, 1024, 3),
                ("rf_rest_1536_bucket", 24, 1008, 2), ("rf_middle_1536_bucket", 24, 252, 2))


def _select(lib, which, case, **knobs):
    entry, Case, Choice = ((lib.sdxl_debug_igemm_select, sc.IgemmCase, sc.IgemmChoice) if which == "igemm" else (lib.sdxl_debug_attn_select, sc.AttnCase, sc.AttnChoice))
    entry.restype, lib.sdxl_last_error.restype = ctypes.c_int, ctypes.c_char_p
    out = Choice()
    status = entry(ctypes.byref(Case(**case)), ctypes.byref(sc.Knobs(**dict(sc.DEFAULT_KNOBS, **knobs))), ctypes.byref(out))
    assert status == 0, (case, lib.sdxl_last_error().decode())
    return out


@pytest.mark.parametrize("name,conv,slices,gn", RF_CONVS)
def test_refiner_block_cases_reach_their_splitk_path(built, name, conv, slices, gn):
    lib = ctypes.CDLL(built.LIB_PATH)
    _, _, _, h, w, _ = R.case(name)
    b = R.block_of(name)
    cin = b["c_out"] if conv == "conv_out" and b["kind"] != "Head" else b["c_in"]      # (a ResBlock's conv_out reads c_out channels; the head's reads the stream)
    rows, stride = (h * w, 1) if conv != "down" else ((h // 2) * (w // 2), 2)
    # the rule's own inputs agree with the table above: rows per entry -> slices wherever K and N let the launch split at all
    splits = 9 * cin >= 10240 and b["c_out"] <= 1536
    assert slices == ({64: 8, 252: 8, 256: 8, 1008: 3, 1024: 3}[rows] if splits else 1), (name, conv, rows, 9 * cin)
    assert gn is (None if not splits else rows % 256 == 0)
    extra = {"conv_in": sc.EBIAS, "conv_out": sc.R if b["kind"] != "Head" else 0, "down": 0}[conv]
    for cdt, adt, odt, present in ((sc.F16, sc.F16, sc.F16, sc.SPLITK_WS | extra), (sc.HL, sc.HL, sc.F32, sc.SPLITK_WS | sc.ACC_SCALE | extra)):
        case = dict(batch=R.B, rows_per_entry=rows, N=b["c_out"], cin=cin, ksize=3, stride=stride, up=0, act=0, n_split=-1, a_dt=adt, c_dt=odt, compute_dt=cdt,
                    xa_nctx=R.N_CTX, shadow_lo_sign=0, present=present, misaligned=0)
        c = _select(lib, "igemm", case)
        print(f"select {name} {conv} compute {cdt}: K {9 * cin} N {b['c_out']} rows {rows} -> family {c.family} tile {c.bm}x{c.bn} splitk {c.splitk} gn_part_ok {c.gn_part_ok}")
        assert c.splitk == slices, (name, conv, cdt, c.splitk)
        if gn is not None:
            assert bool(c.gn_part_ok) == gn, (name, conv, cdt, c.gn_part_ok)
        if gn:      # ... and the launch that carries the statistics is the one selected: 256-row tiles, the same slices
            g = _select(lib, "igemm", dict(case, present=present | sc.GN_PART))
            assert (g.splitk, g.bm) == (slices, 256), (name, conv, cdt, g.splitk, g.bm)
        if slices > 1:
            assert c.bm == 256 and b["c_out"] % c.bn == 0, (name, conv, c.bm, c.bn)      # N = 384 / 768 / 1536: whole column tiles, no 160-wide one


@pytest.mark.parametrize("name,heads,n,kernel", RF_ATTENTION)
def test_refiner_block_cases_reach_their_attention_kernel(built, name, heads, n, kernel):
    lib = ctypes.CDLL(built.LIB_PATH)
    _, _, _, h, w, _ = R.case(name)
    assert (R.block_of(name)["n_head"], h * w) == (heads, n)
    c = _select(lib, "attn", dict(B=R.B, H=heads, Nq=n, Nk=n, dt=sc.F16, present=sc.XSPLIT_WS, misaligned=0))
    print(f"select {name} self-attention: H {heads} queries {n} -> kernel {c.kernel} mix {c.mix} grid {c.grid_x} x {c.grid_y}")
    assert (c.kernel, c.mix) == (kernel, -1)


def test_refiner_head_counts_never_mix_and_do_not_depend_on_the_batch(built):
    """H = 6 / 12 / 24 (not in the recorded table): never the mixed-block kernel, and kernel and mix level are functions of one entry's shape"""
    lib = ctypes.CDLL(built.LIB_PATH)
    cases = [dict(B=B, H=H, Nq=Nq, Nk=Nk, dt=sc.F16, present=ws, misaligned=0) for H in (6, 12, 24) for Nq in (64, 252, 256, 1008, 1024, 4096)
             for Nk in (Nq, 77) for ws in (0, sc.XSPLIT_WS) for B in range(1, 9)]
    rows = [(c.kernel, c.mix) for c in (_select(lib, "attn", case) for case in cases)]
    assert all(k != 4 and m == -1 for k, m in rows)
    n, bad = _batch_dependent([(case, dict(sc.DEFAULT_KNOBS)) for case in cases], rows, "B", lambda r: r)
    assert n == 3 * 6 * 2 * 2 and not bad, bad[:5]
