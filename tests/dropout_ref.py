"""numpy restatement of the dropout mask that include/ucfvit_hip.h defines, shared by the tests/test_dropout_*.py files:

    i = (r * row_step) * D + c                                   (64-bit)
    w = Philox4x32-10(counter = (lo32(i >> 2), hi32(i >> 2), 0, 0), key = (lo32(seed), hi32(seed)))[i & 3]
    dropped iff w < T,  T = min(2^32 - 1, floor(p * 2^32));      kept elements are multiplied by fp32 1 / (1 - p)

Written from the Philox paper's round function (Salmon et al., SC'11), not from the kernel; tests/test_dropout_cpu.py checks it against
the three Random123 known answers."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LO = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """counter words as uint64 arrays holding 32-bit values, key words as Python ints -> the four output words (uint64 arrays < 2^32)"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3))
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                                   # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ np.uint64(k0), p1 & LO, (p0 >> S32) ^ c3 ^ np.uint64(k1), p0 & LO
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def threshold(p):
    return min(2 ** 32 - 1, int(np.floor(np.float64(p) * 2.0 ** 32)))


def words(seed, idx):
    """the 32-bit word of every 64-bit element index in idx (uint64 array)"""
    idx = np.asarray(idx, dtype=np.uint64)
    q = idx >> np.uint64(2)
    w = philox4x32_10(q & LO, q >> S32, np.zeros_like(q), np.zeros_like(q), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    j = idx & np.uint64(3)
    return np.where(j == 0, w[0], np.where(j == 1, w[1], np.where(j == 2, w[2], w[3])))


def keep_mask(seed, rows, D, p, row_step=1, shift=0):
    """bool [rows, D], True = kept; shift: added to every index (the wrong references of the tests)"""
    r = np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(row_step) * np.uint64(D)
    idx = r + np.arange(D, dtype=np.uint64)[None, :] + np.uint64(shift)
    return words(seed, idx) >= np.uint64(threshold(p))


def inv_keep(p):
    """1.0f / (1.0f - p) as the kernel forms it"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
