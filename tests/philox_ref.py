"""numpy restatement of the device generator's contract: Philox4x32-10 words and their
Box-Muller normals, element by element.  The CPU tests check it against the published known-answer vectors; the GPU
tests check cnf_draw_uint32 / cnf_draw_normal against it."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or scalars), key: two uint32 values -> the four output words (uint32 arrays)."""
    c = [np.asarray(x, dtype=np.uint64) for x in ctr]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
    return [x.astype(np.uint32) for x in c]


def _blocks(seed, sub, offset, n):
    """(first block index, the four words of every block covering elements [offset, offset + n))"""
    seed, sub, offset = int(seed), int(sub), int(offset)
    q0, q1 = offset >> 2, (offset + n - 1) >> 2
    q = np.arange(q1 - q0 + 1, dtype=np.uint64) + np.uint64(q0)      # (wraps only past 2**64 blocks: never)
    ctr = [q & MASK, q >> np.uint64(32), np.uint64(sub & 0xFFFFFFFF), np.uint64(sub >> 32)]
    return q0, philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))


def uint32(seed, sub, offset, n):
    """The n words of elements offset .. offset + n - 1."""
    if n == 0:
        return np.zeros(0, np.uint32)
    q0, w = _blocks(seed, sub, offset, n)
    flat = np.stack(w, axis=1).reshape(-1)
    s = int(offset) - 4 * q0
    return flat[s:s + n]


def _sincos_2pi(u):
    """(sin 2 pi u, cos 2 pi u) for u in [0, 1), reduced to an octant exactly (u is a multiple of 2**-32), so that the
    zeros and the values next to them are as accurate as the rest."""
    x = 4.0 * u
    q = np.floor(x)
    f = x - q                                        # exact
    lo = f <= 0.5
    a = np.where(lo, f, 1.0 - f) * (np.pi / 2)
    s = np.where(lo, np.sin(a), np.cos(a))           # sin(pi/2 f), cos(pi/2 f)
    c = np.where(lo, np.cos(a), np.sin(a))
    q = q.astype(np.int64) & 3
    sin = np.select([q == 0, q == 1, q == 2], [s, c, -s], -c)
    cos = np.select([q == 0, q == 1, q == 2], [c, -s, -c], s)
    return sin, cos


def normal64(seed, sub, offset, n):
    """The n normals of elements offset .. offset + n - 1 in float64 (the device rounds each to float32 once)."""
    if n == 0:
        return np.zeros(0)
    q0, w = _blocks(seed, sub, offset, n)
    out = np.empty((len(w[0]), 4))
    for lane in (0, 2):
        u1 = (w[lane].astype(np.float64) + 1.0) * 2.0 ** -32
        u2 = w[lane + 1].astype(np.float64) * 2.0 ** -32
        r = np.sqrt(-2.0 * np.log(u1))
        s, c = _sincos_2pi(u2)
        out[:, lane], out[:, lane + 1] = r * c, r * s
    s = int(offset) - 4 * q0
    return out.reshape(-1)[s:s + n]


def normal(seed, sub, offset, n):
    return normal64(seed, sub, offset, n).astype(np.float32)
