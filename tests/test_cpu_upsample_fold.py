"""The upsample fold (csrc/upsample_fold.h) on the CPU: the algebra in fp64, the library's fp32 sums bit for bit, the host code under sanitizers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import upsample_fold_ref as UF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return pkg


def _weights(cout, cin, seed):
    """fp32 taps with mixed magnitudes and signs, so that the order of the sums shows in the last bit"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((cout, cin, 3, 3)) * np.exp2(rng.integers(-6, 3, (cout, cin, 3, 3)))).astype(np.float32)


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (2, 2, 3), (1, 5, 4), (2, 3, 7)])
def test_phase_convolutions_equal_upsample_then_conv(B, H, W):
    """fp64: every border and corner is a case at 1x1, 2x3 and 5x4 (H != W, B = 2 included)"""
    rng = np.random.default_rng(H * 16 + W)
    x = rng.standard_normal((B, 3, H, W))
    w = rng.standard_normal((4, 3, 3, 3))
    bias = rng.standard_normal(4)
    ref = UF.conv_upsampled(x, w, bias)
    got = UF.conv_phases(x, UF.fold(w, np.float64), bias)
    assert got.shape == ref.shape == (B, 4, 2 * H, 2 * W)
    assert np.abs(got - ref).max() <= 1e-12


def test_library_fold_is_the_stated_fp32_sum(built):
    """sdxl_debug_upsample_fold (the per-element arithmetic of the model builders) == numpy float32, ky major, kx minor, bit for bit"""
    lib = ctypes.CDLL(built.LIB_PATH)
    for cout, cin, seed in ((1, 1, 0), (5, 3, 1), (16, 64, 2)):
        w = _weights(cout, cin, seed)
        out = np.empty((4, cout, cin, 2, 2), np.float32)
        rc = lib.sdxl_debug_upsample_fold(w.ctypes.data_as(ctypes.c_void_p), cout, cin, out.ctypes.data_as(ctypes.c_void_p))
        assert rc == 0
        want = UF.fold(w, np.float32)
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert lib.sdxl_debug_upsample_fold(None, 1, 1, None) != 0


def test_fold_under_sanitizers(tmp_path):
    """csrc/upsample_fold.h + a stand-alone driver built with AddressSanitizer and UBSan; same bits as numpy"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "upsample_fold_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "upsample_fold_driver.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    for cout, cin in ((1, 1), (3, 5), (8, 32)):
        w = _weights(cout, cin, cout)
        src, dst = str(tmp_path / "w.bin"), str(tmp_path / "f.bin")
        with open(src, "wb") as fh:
            fh.write(np.array([cout, cin], np.int32).tobytes() + w.tobytes())
        r = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
        got = np.fromfile(dst, np.float32).reshape(4, cout, cin, 2, 2)
        assert np.array_equal(got.view(np.uint32), UF.fold(w, np.float32).view(np.uint32))
