"""The GEMM / attention kernel selection (csrc/select.cpp) on the CPU: the table of what the launchers chose before the selection
had a home of its own, the batch-independence of every rule that changes output bits, and the host code under sanitizers."""
import collections
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import select_cases as sc

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
