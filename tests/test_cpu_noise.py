"""The numpy Philox4x32-10 that the GPU noise tests compare against, pinned to the published known-answer vectors
(Random123's kat_vectors: counter, key -> output), so the GPU comparison rests on a checked emulation."""
import numpy as np
import pytest

from noise_ref import gen_noise_f64, philox4x32_10

KAT = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answer_vectors(ctr, key, want):
    got = " ".join("%08x" % int(x) for x in philox4x32_10(ctr, key))
    assert got == want


def test_philox_is_vectorised_like_its_scalar_form():
    ctr = [np.array([0, 0x243F6A88], dtype=np.uint64), np.array([0, 0x85A308D3], dtype=np.uint64),
           np.array([0, 0x13198A2E], dtype=np.uint64), np.array([0, 0x03707344], dtype=np.uint64)]
    out = philox4x32_10(ctr, (0, 0))
    assert " ".join("%08x" % int(x[0]) for x in out) == KAT[0][2]


def test_emulated_noise_is_bounded_and_finite():
    z, r, th = gen_noise_f64(0xDEADBEEFCAFEF00D, 3, 16, 15)
    assert z.shape == (4, 16, 15) and np.isfinite(z).all()
    assert np.abs(z).max() <= np.sqrt(48 * np.log(2.0)) and r.min() >= 0 and th.max() < 2 * np.pi
