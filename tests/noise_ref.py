"""Host emulation of the engine's seeded noise, for tests: Philox4x32-10 in numpy, written from the algorithm's definition
(Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC11), and the Box-Muller construction in fp64.

Counter = (hw, draw, 0, 0), key = (seed & 0xffffffff, seed >> 32); output words x0..x3; for p in {0, 1}:
ua = ((x[2p] >> 8) + 1) 2^-24, ub = (x[2p+1] >> 8) 2^-24, r = sqrt(-2 ln ua), theta = 2 pi ub, channel 2p = r cos theta,
channel 2p+1 = r sin theta."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # key increments (golden ratio, sqrt(3) - 1)
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or scalars), key: two Python ints -> four uint64 arrays holding the 32-bit output words"""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in ctr]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]          # 32 x 32 -> 64, no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def noise_words(seed: int, draw: int, hw_count: int):
    hw = np.arange(hw_count, dtype=np.uint64)
    z = np.zeros_like(hw)
    return philox4x32_10((hw, z + np.uint64(draw), z, z), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def gen_noise_f64(seed: int, draw: int, h: int, w: int):
    """-> (z [4, h, w] fp64, r [4, h, w], theta [4, h, w]): the exact-arithmetic value of every element with the radius and
    angle it was built from (the error bar of the device values is a function of both)"""
    x = noise_words(seed, draw, h * w)
    z, rr, tt = np.empty((4, h * w)), np.empty((4, h * w)), np.empty((4, h * w))
    for p in range(2):
        ua = ((x[2 * p] >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        ub = (x[2 * p + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        r, th = np.sqrt(-2.0 * np.log(ua)), 2.0 * np.pi * ub
        z[2 * p], z[2 * p + 1] = r * np.cos(th), r * np.sin(th)
        rr[2 * p] = rr[2 * p + 1] = r
        tt[2 * p] = tt[2 * p + 1] = th
    return z.reshape(4, h, w), rr.reshape(4, h, w), tt.reshape(4, h, w)
