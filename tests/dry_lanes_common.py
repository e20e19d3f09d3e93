"""Inputs whose channels code at very different bit rates, shared by tests/test_kernel_sim_dry_lanes.py (emulator) and
tests/test_gpu_dry_lanes.py (GPU).  The encoder's filling wave works in row lockstep, so within a wave every lane below the
highest rate has no word queued in many of the coding wave's steps ("dry lanes"); such steps take the masked steady word
path with the dry lanes coding an empty part (dega_kernels.hpp, encode_coding_wave).  Every channel of every case is held
to oracle.orc.encode_i32 byte for byte: stream, bit count and status, which is 0 for all of them."""
import numpy as np

from oracle import orc


def walk(rng, T, amp, base):
    """a random walk with uniform steps in [-amp, amp] around `base`, as int64 (amp 0: a constant)"""
    if amp == 0:
        return np.full(T, base, dtype=np.int64)
    return np.cumsum(rng.integers(-amp, amp + 1, T)) + base


def from_amplitudes(amps, T, seed, base=100_000_000):
    """[T, C] int32, channel c a walk of amplitude amps[c]; every sample stays within [0, 2^31) (checked)"""
    rng = np.random.default_rng(seed)
    x = np.stack([walk(rng, T, int(a), base) for a in amps], axis=1)
    assert x.min() >= 0 and x.max() < 2 ** 31
    return np.ascontiguousarray(x.astype(np.int32))


def mixed_rates(Cn=64, T=3000, seed=1):
    """(a) of every 64 channels: 16 constant, 16 walk +-3, 16 walk +-50, 16 walk +-3 000 -- most lanes dry most of the time"""
    return from_amplitudes([(0, 3, 50, 3000)[(c % 64) // 16] for c in range(Cn)], T, seed)


def one_heavy_lane(Cn=64, T=3000, seed=2, heavy=37):
    """(b) equal-rate lanes and one that needs many times their bits"""
    return from_amplitudes([30000 if c % 64 == heavy else 50 for c in range(Cn)], T, seed)


def ragged(Cn=100, T=3000, seed=3):
    """(c) mixed rates again, interleaved this time, in a channel count of the caller's choice (100: a ragged last wave)"""
    return from_amplitudes([(50, 0, 3000, 3)[c % 4] for c in range(Cn)], T, seed)


def halving_with_dry_lanes(Cn=64, T=2000, seed=4):
    """(f) walks of +-40 .. +-55 reach cum[0] = 16383 (some 13 symbols per sample: T >= 1 700) at a different step each, a
    few constant channels and a few fast ones beside them: a lane at its halving (CLS_SPLIT) and dry lanes meet in one step"""
    return from_amplitudes([0 if c % 16 == 0 else (3000 if c % 16 == 9 else 40 + c % 16) for c in range(Cn)], T, seed)


_oracle_cache = {}


def oracle_streams(key, x, adaptive):
    """[(status, bytes, bits)] per channel from orc.encode_i32, computed once per (key, adaptive)"""
    k = (key, adaptive)
    if k not in _oracle_cache:
        _oracle_cache[k] = [orc.encode_i32(np.ascontiguousarray(x[:, c]), adaptive) for c in range(x.shape[1])]
    return _oracle_cache[k]


def assert_equals_oracle(key, x, adaptive, out, bits, err, tag=None):
    want = oracle_streams(key, x, adaptive)
    for c, (status, data, n) in enumerate(want):
        assert status == 0, (tag or key, c, "the case is meant to code cleanly")
        assert int(err[c]) == 0, (tag or key, c, int(err[c]))
        assert int(bits[c]) == n, (tag or key, c, int(bits[c]), n)
        assert out[c, : (n + 7) // 8].tobytes() == data, (tag or key, c)
