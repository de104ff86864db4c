"""The device generator's contract without a GPU: the numpy restatement (tests/philox_ref.py)
against the published Philox4x32-10 known-answer vectors, the properties the GPU tests lean on, and the host side of
HIPRNG."""
import numpy as np
import pytest

import continuousnf.jl_amd as cnf
from tests import philox_ref as P

F = 0xFFFFFFFF


@pytest.mark.parametrize("ctr,key,out", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((F, F, F, F), (F, F), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_known_answer_vectors(ctr, key, out):
    got = P.philox4x32_10([np.uint32(c) for c in ctr], key)
    assert [int(w) for w in got] == list(out)


def test_element_layout_follows_the_counter_and_key():
    """Element e of (seed, sub) is word e & 3 of Philox(ctr = (q_lo, q_hi, sub_lo, sub_hi), key = (seed_lo, seed_hi))."""
    seed, sub = 0x0123456789ABCDEF, (1 << 63) + 5
    for e in (0, 3, 6, 4 * 2 ** 32 + 1, 2 ** 40 + 1):
        q = e >> 2
        w = P.philox4x32_10([np.uint32(q & F), np.uint32(q >> 32), np.uint32(sub & F), np.uint32(sub >> 32)],
                            (seed & F, seed >> 32))
        assert int(P.uint32(seed, sub, e, 1)[0]) == int(w[e & 3])


@pytest.mark.parametrize("offset", [0, 1, 3, 5, 4 * 2 ** 32 - 6])
def test_stream_splits_into_consecutive_pieces(offset):
    seed, sub, n = 7, 3, 1001
    whole_u, whole_n = P.uint32(seed, sub, offset, n), P.normal64(seed, sub, offset, n)
    cuts = [0, 1, 2, 7, 8, 13, 400, 999, n]
    parts_u = [P.uint32(seed, sub, offset + a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    parts_n = [P.normal64(seed, sub, offset + a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(whole_u, np.concatenate(parts_u))
    # (the words are exact; the float64 normals may differ in their last bit between numpy's SIMD and scalar loops)
    np.testing.assert_allclose(np.concatenate(parts_n), whole_n, rtol=1e-15, atol=1e-15)


def test_box_muller_pairs_and_the_end_of_the_unit_interval():
    """Lanes (0, 1) and (2, 3) of a block are one Box-Muller pair each; w_even = 2^32 - 1 gives u1 = 1 exactly, r = 0."""
    w = P.uint32(11, 0, 0, 8).astype(np.float64)
    z = P.normal64(11, 0, 0, 8)
    for k in range(0, 8, 2):
        r = np.sqrt(-2 * np.log((w[k] + 1) * 2.0 ** -32))
        assert np.isclose(z[k], r * np.cos(2 * np.pi * w[k + 1] * 2.0 ** -32), rtol=1e-12, atol=1e-15)
        assert np.isclose(z[k + 1], r * np.sin(2 * np.pi * w[k + 1] * 2.0 ** -32), rtol=1e-12, atol=1e-15)
    s, c = P._sincos_2pi(np.array([0.0, 0.25, 0.5, 0.75, 0.125]))
    assert np.array_equal(s[:4], [0.0, 1.0, 0.0, -1.0]) and np.array_equal(np.abs(c[:4]), [1.0, 0.0, 1.0, 0.0])
    assert np.isclose(s[4], np.sqrt(0.5), rtol=1e-15) and np.isclose(c[4], np.sqrt(0.5), rtol=1e-15)


def test_streams_differ_by_seed_and_subsequence():
    a = P.uint32(1, 0, 0, 64)
    assert not np.array_equal(a, P.uint32(2, 0, 0, 64))
    assert not np.array_equal(a, P.uint32(1, 1, 0, 64))


def test_hiprng_offset_and_state():
    r = cnf.HIPRNG(2 ** 64 - 1, subsequence=3)
    assert (r.seed, r.subsequence, r.offset) == (2 ** 64 - 1, 3, 0)
    assert r.take(10) == 0 and r.take(5) == 10 and r.offset == 15
    st = r.get_state()
    u1 = r.uniform(-1, 1)
    r.take(7)
    r.set_state(st)
    assert r.offset == 15 and r.uniform(-1, 1) == u1
    with pytest.raises(ValueError):
        cnf.HIPRNG(-1)
    with pytest.raises(ValueError):
        cnf.HIPRNG(2 ** 64)
    r.offset = 2 ** 64 - 2
    with pytest.raises(ValueError):
        r.take(2)


def test_hiprng_host_draws_are_seeded():
    a, b = cnf.HIPRNG(5), cnf.HIPRNG(5)
    assert a.uniform(-0.5, 0.5) == b.uniform(-0.5, 0.5)
    assert np.array_equal(a.permutation(100), b.permutation(100))
    assert not np.array_equal(cnf.HIPRNG(6).permutation(100), cnf.HIPRNG(5).permutation(100))
    assert a.offset == 0                              # host draws take no device elements


def test_construct_keeps_host_generators_and_accepts_hiprng():
    nn = cnf.Chain(cnf.Dense(2, 6, "tanh"), cnf.Dense(6, 2, "tanh"))
    assert isinstance(cnf.construct(cnf.RNODE, nn, 1, 1, rng=3).rng, np.random.Generator)
    assert isinstance(cnf.construct(cnf.RNODE, nn, 1, 1).rng, np.random.Generator)
    g = np.random.default_rng(1)
    assert cnf.construct(cnf.RNODE, nn, 1, 1, rng=g).rng is g
    h = cnf.HIPRNG(4)
    ic = cnf.construct(cnf.RNODE, nn, 1, 1, rng=h)
    assert ic.rng is h
    ps, st = cnf.setup(ic.rng, nn)                    # fit's parameter initialisation draws on the host side
    assert ps.dtype == np.float32 and np.array_equal(ps, cnf.setup(cnf.HIPRNG(4), nn)[0])
    assert h.offset == 0


def test_draw_entry_points_validate_before_touching_the_device():
    """n = 0 is a no-op (NULL out allowed); NULL out, a misaligned out or offset + n past 2^64 - 1 are refused."""
    from continuousnf.jl_amd import _lib
    l = _lib.lib()
    for fn in (l.cnf_draw_normal, l.cnf_draw_uint32):
        assert fn(0, 1, 0, 0, None, 0, None) == _lib.OK
        assert fn(0, 1, 0, 2 ** 64 - 1, None, 0, None) == _lib.OK
        assert fn(0, 1, 0, 0, None, 4, None) == _lib.ERR_BAD_ARG
        assert fn(0, 1, 0, 2 ** 64 - 4, 4096, 5, None) == _lib.ERR_BAD_ARG      # (never dereferenced)
        assert fn(0, 1, 0, 0, 4098, 5, None) == _lib.ERR_BAD_ARG               # not 4-byte aligned
