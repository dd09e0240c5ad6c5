"""TEST INFRASTRUCTURE: the stream of csrc/coarse_draw.hip restated in numpy from the statement in include/sugar_raster.h
(sgr_draw_samples): Philox4x32-10 with the standard constants, the key (seed lo32, seed hi32), two blocks per sample with the
counters (c lo32, c hi32, call lo32, call hi32), c = 2 n and 2 n + 1; block 0 gives the index word and one Box-Muller pair, block 1
the pair whose cosine branch is the third normal.  The indices are integers and restated exactly; the normals are evaluated in the
dtype asked for: float64 is the truth, float32 (numpy's correctly rounded-or-close log / sin / cos, every operation rounded on its
own) gives the yard."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two; returns uint32 [..., 4]"""
    c = [np.atleast_1d(np.asarray(w, dtype=np.uint64)) & _MASK for w in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (int(key[0]) & 0xFFFFFFFF), (int(key[1]) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]          # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _MASK, p1 >> np.uint64(32), p1 & _MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, -1).astype(np.uint32)


def sample_words(n_samples, seed, call):
    """(block0 uint32[N,4], block1 uint32[N,4]) of the samples 0 .. N-1"""
    seed, call = int(seed) & (2 ** 64 - 1), int(call) & (2 ** 64 - 1)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    c = 2 * np.arange(n_samples, dtype=np.uint64)
    blocks = []
    for cc in (c, c + np.uint64(1)):
        blocks.append(philox4x32_10((cc & _MASK, cc >> np.uint64(32), call & 0xFFFFFFFF, call >> 32), key))
    return blocks[0], blocks[1]


def pick(r0, n_masked):
    """j = (uint64(r0) * n_masked) >> 32"""
    return ((r0.astype(np.uint64) * np.uint64(n_masked)) >> np.uint64(32)).astype(np.int64)


def unit_open(r, dtype):
    """u = ((r >> 8) + 0.5) * 2^-24 in `dtype`"""
    return ((r >> np.uint32(8)).astype(dtype) + dtype(0.5)) * dtype(2.0 ** -24)


def box_muller(ra, rb, dtype):
    """(rho cos(theta), rho sin(theta)) with rho = sqrt(-2 log u(ra)), theta = 2 pi u(rb), in `dtype`"""
    rho = np.sqrt(dtype(-2.0) * np.log(unit_open(ra, dtype)))
    theta = dtype(6.283185307179586) * unit_open(rb, dtype)
    return rho * np.cos(theta), rho * np.sin(theta)


def normals(n_samples, seed, call, dtype=np.float64):
    """noise[N,3] of the stream in `dtype`"""
    a, b = sample_words(n_samples, seed, call)
    z0, z1 = box_muller(a[:, 1], a[:, 2], dtype)
    z2, _ = box_muller(b[:, 0], b[:, 1], dtype)
    return np.stack((z0, z1, z2), -1)


def draw_samples(mask, n_samples, seed, call, dtype=np.float64):
    """(sample_idx int64[N], noise [N,3] in `dtype`, n_masked) of sgr_draw_samples for a numpy bool mask"""
    mask = np.asarray(mask, dtype=bool)
    ids = np.flatnonzero(mask)
    if len(ids) == 0:
        return np.zeros(n_samples, np.int64), np.zeros((n_samples, 3), dtype), 0
    a, _ = sample_words(n_samples, seed, call)
    return ids[pick(a[:, 0], len(ids))].astype(np.int64), normals(n_samples, seed, call, dtype), len(ids)
