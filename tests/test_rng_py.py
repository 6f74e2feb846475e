"""bppo.rng.StdRng (pure Python, the opponent pool's sampler) against the oracle's RNG
(oracle/rng.c, pinned by tests/test_oracle_rng.py) and the library's host draw chain."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_ffi as O
from bppo.rng import StdRng, chacha_block, seed_key

SEEDS = (0, 42, 2**64 - 1)


@pytest.mark.parametrize("seed", SEEDS)
def test_key_and_words_match_oracle(seed):
    assert seed_key(seed) == [int(k) for k in O.seed_key(seed)]
    r, o = StdRng.seed_from_u64(seed), O.new_rng(seed)
    for _ in range(100):
        assert r.next_u32() == O.lib().or_rng_next_u32(C.byref(o))
    assert r.pos == 100 == o.word_pos


def test_chacha12_block_matches_oracle():
    key = seed_key(42)
    for counter in (0, 1, 2**32 - 1, 2**32, 2**40 + 7):
        assert chacha_block(key, counter) == [int(w) for w in O.chacha_block(key, counter, 0, rounds=12)]


@pytest.mark.parametrize("seed", SEEDS)
def test_next_u64_matches_oracle_across_block_ends(seed):
    r, o = StdRng.seed_from_u64(seed), O.new_rng(seed)
    # 15 u32 first: the next u64 takes word 15 of block 0 and word 0 of block 1
    for _ in range(15):
        assert r.next_u32() == O.lib().or_rng_next_u32(C.byref(o))
    straddled = False
    for _ in range(100):
        straddled |= r.pos % 16 == 15
        assert r.next_u64() == O.lib().or_rng_next_u64(C.byref(o))
    assert straddled and r.pos == o.word_pos
    # mixed widths stay in step
    for i in range(100):
        if i % 3:
            assert r.next_u64() == O.lib().or_rng_next_u64(C.byref(o))
        else:
            assert r.next_u32() == O.lib().or_rng_next_u32(C.byref(o))


def _widening_u64(words, n):
    """UniformInt<u64>::sample_single on a list of u32 words -> (value, words used)"""
    zone = ((n << (64 - n.bit_length())) - 1) & (2**64 - 1)
    i = 0
    while True:
        v = int(words[i]) | (int(words[i + 1]) << 32)
        i += 2
        m = v * n
        if (m & (2**64 - 1)) <= zone:
            return m >> 64, i


@pytest.mark.parametrize("seed", SEEDS)
def test_gen_range_usize(seed):
    words = O.stdrng_words(seed, 4000)
    r, o = StdRng.seed_from_u64(seed), O.new_rng(seed)
    pos = 0
    for n in [1, 2, 3, 4, 5, 6, 7, 15, 16, 17, 1000, 2**31 + 1, 2**33 + 5, 2**63 + 1] * 20:
        want, used = _widening_u64(words[pos:], n)
        pos += used
        assert r.gen_range(n) == want
        assert want == O.lib().or_gen_range_u64(C.byref(o), 0, n)
        assert r.pos == pos == o.word_pos
    assert pos > 2 * 14 * 20            # some draw was rejected (2^63 + 1 rejects about half)


@pytest.mark.parametrize("seed", SEEDS)
def test_gen_f64(seed):
    r, o = StdRng.seed_from_u64(seed), O.new_rng(seed)
    for _ in range(50):
        v = O.lib().or_rng_next_u64(C.byref(o))
        x = r.gen_f64()
        assert x == (v >> 11) * 2.0**-53 and 0.0 <= x < 1.0


def _libbppo():
    import bppo._lib as L
    return L.lib() if os.path.exists(L.LIB_PATH) else None


@pytest.mark.parametrize("seed,pos,n", [(0, 0, 300), (42, 7, 1000), (2**64 - 1, 12345, 257)])
def test_shuffle_draws(seed, pos, n):
    """SliceRandom::shuffle's draws J[i] = gen_range(0..i + 1), i = n - 1 .. 1 (u32 sampling)"""
    lib = _libbppo()
    r = StdRng(seed_key(seed), pos)
    mine = {i: r.gen_range_u32(i + 1) for i in range(n - 1, 0, -1)}
    if lib is not None:                 # the library's host draw chain (no GPU involved)
        J = np.zeros(n, np.uint32)
        end = C.c_uint64()
        assert lib.bppo_debug_shuffle_chain(seed, 0, pos, n, J.ctypes.data, C.byref(end)) == 0
        assert end.value == r.pos
        assert all(int(J[i]) == mine[i] for i in range(1, n))
    o = O.new_rng(seed)
    o.word_pos = pos
    for i in range(n - 1, 0, -1):
        assert O.lib().or_gen_range_u32(C.byref(o), 0, i + 1) == mine[i]
    assert o.word_pos == r.pos


def test_shuffle_matches_oracle():
    for seed in SEEDS:
        r, o = StdRng.seed_from_u64(seed), O.new_rng(seed)
        a = list(range(37))
        b = np.arange(37, dtype=np.uint32)
        r.shuffle(a)
        O.lib().or_shuffle_u32(C.byref(o), b, b.size)
        assert a == [int(x) for x in b] and r.pos == o.word_pos
