"""numpy restatement of the in-kernel dropout contract (include/lipvq.h, "in-kernel dropout"): Philox4x32-10 and the mapping from
(seed, step, site, row, col) to a keep decision.  Written from the published algorithm (Salmon et al., SC'11), not from
csrc/lipvq_rng.h: tests/test_dropout_host.py holds the library's host function to it byte for byte."""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two ints -> four uint32 arrays."""
    c = [np.asarray(w, dtype=np.uint64) & np.uint64(MASK32) for w in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]                       # (32 x 32 -> 64 bits: exact in uint64)
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK32)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK32)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return [w.astype(np.uint32) for w in c]


def threshold(p):
    assert 0.0 < p < 1.0
    return int(math.floor(p * 4294967296.0))


def inv_keep(p):
    return np.float32(1.0) / np.float32(1.0 - p)


def keep_field(seed, step, site, rows, cols, p, row0=0):
    """uint8 [rows, cols]: 1 where element (row0 + row, col) of the site is kept (row0: a window of a larger field)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    row = np.arange(int(row0), int(row0) + rows, dtype=np.uint64)[:, None]
    col = np.arange(cols, dtype=np.uint64)[None, :]
    words = philox4x32_10((col >> np.uint64(2), row, int(site), int(step) & MASK32), (seed & MASK32, seed >> 32))
    pick = np.broadcast_to(col & np.uint64(3), (rows, cols))
    word = np.choose(pick.astype(np.int64), [np.broadcast_to(w, (rows, cols)) for w in words])
    return (word >= np.uint32(threshold(p))).astype(np.uint8)
