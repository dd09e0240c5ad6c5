"""The kernels whose prefix sums go through csrc/sgr_device.h (sgr_wave_incl_scan / sgr_block_scan), at lengths that cross a wave (64)
and a workgroup boundary, against torch on the device.  Everything compared is an integer (or an integer-valued float): equality is exact.
Marching cubes and the binning kernels have fixed shapes and are held by their own suites."""
import ctypes as C

import pytest
import torch

from sugar_amd import _lib
from sugar_amd._call import call, ptr
from sugar_amd.knn import knn_points

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [1, 63, 64, 65, 255, 256, 257, 2049, 4097]


def _scatter_rows(n):
    """the k_fscan_* chain of csrc/group.hip: sgr_scatter_add_rows groups n entries by row with a radix sort whose digit offsets are that scan"""
    g = torch.Generator().manual_seed(n)
    P = n                                                       # the row count crosses the same boundaries
    ix = torch.randint(0, P, (n,), generator=g).to(DEV)
    val = (torch.arange(n) % 7 + 1).to(torch.float32).to(DEV).reshape(n, 1)      # small integers: float addition is exact
    out = torch.empty(P, 1, dtype=torch.float32, device=DEV)
    scratch = torch.empty(_lib.load().sgr_scatter_add_rows_scratch_bytes(n, P), dtype=torch.uint8, device=DEV)
    call("sgr_scatter_add_rows", DEV, n, ptr(ix), ptr(val), 1, P, ptr(out), ptr(scratch))
    want = torch.zeros(P, 1, dtype=torch.float32, device=DEV).index_add_(0, ix, val)
    assert torch.equal(out, want)
    counts = torch.bincount(ix, minlength=P)
    ones = torch.ones(n, 1, dtype=torch.float32, device=DEV)
    call("sgr_scatter_add_rows", DEV, n, ptr(ix), ptr(ones), 1, P, ptr(out), ptr(scratch))
    assert torch.equal(torch.cumsum(out[:, 0].to(torch.int64), 0), torch.cumsum(counts, 0))


def _knn_grid(n):
    """the grid's cell starts (k_grid_blocksum / k_grid_scan, and the row walk of the query kernel): neighbours against brute force"""
    g = torch.Generator().manual_seed(1000 + n)
    pts = torch.rand(n, 3, generator=g).to(DEV)
    K = min(4, n)
    got = knn_points(pts[None], pts[None], K=K, method="grid")
    exhaustive = knn_points(pts[None], pts[None], K=K, method="brute")           # the LDS-tiled kernel: no grid, no scan
    assert torch.equal(got.idx, exhaustive.idx) and torch.equal(got.dists, exhaustive.dists)
    d2 = ((pts.double()[:, None, :] - pts.double()[None, :, :]) ** 2).sum(-1)
    want_d, want_i = torch.topk(d2, K, dim=1, largest=False, sorted=True)
    idx = got.idx[0]
    # float32 squared distances carry a few ulp (three products, two sums: below 1e-6 relative); two neighbours closer than that in
    # distance may swap places, any other difference is an error
    same = idx == want_i
    picked_d = torch.gather(d2, 1, idx)
    assert bool((same | ((picked_d - want_d).abs() <= 1e-6 * want_d)).all())
    assert bool(same[:, 0].all())                      # every point is its own nearest neighbour, at distance 0
    assert torch.allclose(got.dists[0].double(), picked_d, rtol=1e-5, atol=1e-12)


def _pick(n):
    """sgr_pick_pixels on an n-pixel depth map: k >= the valid pixels returns exactly those, in raster order (k_pick_count / k_pick_scan
    / k_pick_write); a smaller k returns k of them, ascending (k_pick_select's scan finds the threshold)"""
    lib = _lib.load()
    g = torch.Generator().manual_seed(2000 + n)
    depth = torch.where(torch.rand(n, generator=g) < 0.6, torch.rand(n, generator=g) + 0.5, torch.full((n,), -1.0)).to(DEV)
    valid = torch.nonzero(depth >= 0)[:, 0]
    n_valid = int(valid.numel())
    scratch = torch.empty(int(lib.sgr_pick_pixels_scratch_bytes(n)), dtype=torch.uint8, device=DEV)
    for k in sorted({n, max(1, n_valid // 2)}):
        picked = torch.full((k,), -7, dtype=torch.int64, device=DEV)
        words = torch.zeros(2, dtype=torch.int32, device=DEV)
        call("sgr_pick_pixels", DEV, n, ptr(depth), k, C.c_uint32(12345), ptr(picked), ptr(words), C.c_void_p(words.data_ptr() + 4),
             ptr(scratch))
        count, seen_valid = words.tolist()
        assert seen_valid == n_valid and count == min(k, n_valid)
        got = picked[:count]
        if k >= n_valid:
            assert torch.equal(got, valid)
        else:
            assert bool((got[1:] > got[:-1]).all()) and bool(torch.isin(got, valid).all())


@pytest.mark.parametrize("n", SIZES)
def test_scans_match_torch_exactly(n):
    _scatter_rows(n)
    _knn_grid(n)
    _pick(n)


def test_pick_block_starts_across_waves_and_rounds():
    """SIZES give k_pick_scan at most 5 block counts (1024 pixels per block): one wave, one round.  1025 blocks put its sum over the
    earlier waves and the carry from the first round of 1024 into the second to work."""
    _pick(1024 * 1024 + 1)
