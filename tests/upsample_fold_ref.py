"""The upsample fold in numpy, shared by the CPU and the GPU tests: nearest-2x upsample + padded 3x3 convolution == four 2x2-tap phase
convolutions on the source.  Output pixel (2i + a, 2j + b) has phase (a, b); W_ab[dy][dx] = sum over ky in R_a(dy), kx in R_b(dx) of w[ky][kx];
tap (dy, dx) reads source pixel (i + dy - 1 + a, j + dx - 1 + b), zero outside the source."""
import numpy as np

R = {0: ([0], [1, 2]), 1: ([0, 1], [2])}      # R[a][d] = taps of the 3-window that land on source offset d


def fold(w, dtype):
    """w [Cout, Cin, 3, 3] -> [4, Cout, Cin, 2, 2] (phase = 2a + b), summed in `dtype` in the one stated order: ky major, kx minor"""
    w = np.asarray(w, dtype=dtype)
    out = np.zeros((4,) + w.shape[:2] + (2, 2), dtype=dtype)
    for a in (0, 1):
        for b in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    acc = None
                    for ky in R[a][dy]:
                        for kx in R[b][dx]:
                            acc = w[:, :, ky, kx].copy() if acc is None else (acc + w[:, :, ky, kx]).astype(dtype)
                    out[2 * a + b, :, :, dy, dx] = acc
    return out


def conv_upsampled(x, w, bias=None):
    """fp64: nearest-2x upsample of x [B, Cin, H, W], then the 3x3 convolution with pad 1 -> [B, Cout, 2H, 2W]"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    up = x.repeat(2, axis=2).repeat(2, axis=3)
    B, _, H2, W2 = up.shape
    pad = np.zeros((B, up.shape[1], H2 + 2, W2 + 2))
    pad[:, :, 1:-1, 1:-1] = up
    out = np.zeros((B, w.shape[0], H2, W2))
    for ky in range(3):
        for kx in range(3):
            out += np.einsum("bchw,oc->bohw", pad[:, :, ky:ky + H2, kx:kx + W2], w[:, :, ky, kx])
    return out if bias is None else out + np.asarray(bias, np.float64)[None, :, None, None]


def conv_phases(x, wf, bias=None):
    """fp64: the four 2x2-tap phase convolutions of folded weights wf [4, Cout, Cin, 2, 2] on x -> [B, Cout, 2H, 2W]"""
    x, wf = np.asarray(x, np.float64), np.asarray(wf, np.float64)
    B, _, H, W = x.shape
    pad = np.zeros((B, x.shape[1], H + 2, W + 2))
    pad[:, :, 1:-1, 1:-1] = x
    out = np.zeros((B, wf.shape[1], 2 * H, 2 * W))
    for a in (0, 1):
        for b in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    # source pixel (i + dy - 1 + a, j + dx - 1 + b) = padded index (i + dy + a, j + dx + b)
                    out[:, :, a::2, b::2] += np.einsum("bchw,oc->bohw", pad[:, :, dy + a:dy + a + H, dx + b:dx + b + W], wf[2 * a + b, :, :, dy, dx])
    return out if bias is None else out + np.asarray(bias, np.float64)[None, :, None, None]
