"""NumPy float64 reference of the posterior draws (include/pmf_hip.h, pmf_gauss_sample_rows): Philox4x32-10 on the counter
(row id, draw index, k // 4, side) under the key (seed low, seed high), the double Box-Muller, and draws m + chol(V) z by
`np.linalg.cholesky`.  Written from the header's definition alone; shares no code with the library."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
TWO_PI = 6.283185307179586


def philox4x32_10(counter, key):
    """counter: uint64 array [..., 4] of 32-bit words, key: (k0, k1) -> uint64 array [..., 4] of output words"""
    c = np.array(counter, dtype=np.uint64) & np.uint64(MASK)
    c0, c1, c2, c3 = (c[..., w].copy() for w in range(4))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & np.uint64(MASK), n2, p0 & np.uint64(MASK)
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack([c0, c1, c2, c3], axis=-1)


def words(seed, side, rows, draws, blocks):
    """uint64 [len(rows), len(draws), len(blocks), 4]: the stream's words; `blocks` = the block numbers, or their count n
    for 0 .. n - 1"""
    rows, draws = np.asarray(rows, dtype=np.uint64).reshape(-1), np.asarray(draws, dtype=np.uint64).reshape(-1)
    blocks = np.arange(blocks, dtype=np.uint64) if np.ndim(blocks) == 0 else np.asarray(blocks, dtype=np.uint64).reshape(-1)
    ctr = np.zeros((len(rows), len(draws), len(blocks), 4), dtype=np.uint64)
    ctr[..., 0] = rows[:, None, None]
    ctr[..., 1] = draws[None, :, None]
    ctr[..., 2] = blocks[None, None, :]
    ctr[..., 3] = np.uint64(side)
    seed = int(seed)
    return philox4x32_10(ctr, (seed & MASK, (seed >> 32) & MASK))


def box_muller(w):
    """words [..., 4] -> normals [..., 4] in float64"""
    u = (w.astype(np.float64) + 0.5) * 2.0 ** -32
    z = np.empty(w.shape, dtype=np.float64)
    for h in (0, 2):
        r = np.sqrt(-2.0 * np.log(u[..., h]))
        a = TWO_PI * u[..., h + 1]
        z[..., h], z[..., h + 1] = r * np.cos(a), r * np.sin(a)
    return z


def normals(seed, side, rows, draws, K):
    """float64 [len(rows), len(draws), K]: z_k of (seed, side, row, draw index)"""
    nb = (K + 3) // 4
    z = box_muller(words(seed, side, rows, draws, nb))
    return z.reshape(z.shape[0], z.shape[1], nb * 4)[:, :, :K]


def draws(m, V, z):
    """m [n, K], V [n, K, K], z [n, D, K] -> m + chol(V) z, [n, D, K]"""
    C = np.linalg.cholesky(V)
    return m[:, None, :] + np.einsum("nij,ndj->ndi", C, z)
