"""GPU pins of the coarse stage's device-side sample draws (sugar_amd.coarse_draw over csrc/coarse_draw.hip) against the numpy
restatement of the stream (tests/coarse_draw_restatement.py, from the statement in include/sugar_raster.h):

  * `sample_idx` and `n_masked` bit for bit: P in {1, 255, 256, 257, 70 000} (70 000 > 65 536 and spans many workgroups of the
    compaction), N in {1, 257, 4 097}; masks of about half density, a single True at row 0 and at row P - 1, and all True.
  * `noise` against the float64 restatement from the same words: norm-wise within max(4 x yard, 1e-6), the yard being the distance of
    the numpy float32 evaluation of the same formulas from float64 (the rule of tests/test_gpu_coarse_loss.py).
  * an all-False mask: n_masked = 0 and zeros; the same (seed, call) gives the same bits, call + 1 other rows; no host synchronisation.
Each noise check prints its distance, its bar and its ratio to the yard."""
import numpy as np
import pytest
import torch

from sugar_amd import coarse_draw
from tests import coarse_draw_restatement as cd
from tests import sdf_regulariser_restatement as rs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 1e-6
SIZES_P = (1, 255, 256, 257, 70_000)
SIZES_N = (1, 257, 4_097)
SEED, CALL = 0x1234_5678_9ABC_DEF0, (1 << 32) + 7          # both halves of the key and of the call words in use


def _masks(P):
    g = np.random.default_rng(P)
    half = g.random(P) < 0.5
    if not half.any():
        half[0] = True
    first, last = np.zeros(P, bool), np.zeros(P, bool)
    first[0], last[P - 1] = True, True
    return dict(half=half, first=first, last=last, all=np.ones(P, bool))


def _draw(mask, N, seed=SEED, call=CALL):
    idx, noise, nm = coarse_draw.draw_samples(torch.as_tensor(mask).to(DEV), N, seed, call)
    assert idx.dtype == torch.int64 and idx.shape == (N,) and noise.dtype == torch.float32 and noise.shape == (N, 3)
    assert nm.dtype == torch.int64 and nm.dim() == 0 and nm.device.type == "cuda"
    return idx, noise, nm


@pytest.mark.parametrize("P", SIZES_P)
def test_indices_and_count_are_the_restatement_bit_for_bit(P):
    for kind, mask in _masks(P).items():
        for N in SIZES_N:
            idx, _, nm = _draw(mask, N)
            want_idx, _, want_nm = cd.draw_samples(mask, N, SEED, CALL)
            assert int(nm) == want_nm == int(mask.sum()), (P, kind, N)
            assert np.array_equal(idx.cpu().numpy(), want_idx), (P, kind, N)
            assert mask[idx.cpu().numpy()].all()


@pytest.mark.parametrize("N", SIZES_N)
def test_noise_is_within_the_float32_yard_of_the_float64_restatement(N):
    mask = _masks(257)["half"]
    _, noise, _ = _draw(mask, N)
    want = cd.normals(N, SEED, CALL, np.float64)
    yard = rs.distance(cd.normals(N, SEED, CALL, np.float32), want)
    d = rs.distance(noise, want)
    bar = max(4.0 * yard, FLOOR)
    print(f"noise N={N:5d}   distance {d:.3e}   bar {bar:.3e}   yard {yard:.3e}   ratio-to-yard {d / max(yard, 1e-30):.2f}")
    assert torch.isfinite(noise).all()
    assert d <= bar, (N, d, bar)


def test_the_noise_does_not_depend_on_the_mask():
    a = _draw(_masks(257)["half"], 4097)[1]
    b = _draw(_masks(70_000)["all"], 4097)[1]
    assert torch.equal(a, b)


def test_an_all_false_mask_gives_zero_count_and_zeros():
    for P in (1, 257, 70_000):
        idx, noise, nm = _draw(np.zeros(P, bool), 4097)
        assert int(nm) == 0 and not idx.any() and not noise.any()


def test_same_seed_and_call_same_bits_next_call_other_rows():
    mask = _masks(70_000)["half"]
    N = 4097
    a, b = _draw(mask, N), _draw(mask, N)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    c = _draw(mask, N, call=CALL + 1)
    assert float(((c[0] != a[0]) | (c[1] != a[1]).any(-1)).float().mean()) > 0.99
    assert float((c[1] != a[1]).all(-1).float().mean()) > 0.99
    d = _draw(mask, N, seed=SEED + 1)
    assert float((d[1] != a[1]).all(-1).float().mean()) > 0.99


def test_argument_checks():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        coarse_draw.draw_samples(torch.ones(4, dtype=torch.bool), 4, 0, 0)
    with pytest.raises(RuntimeError, match="bool"):
        coarse_draw.draw_samples(torch.ones(4, device=DEV), 4, 0, 0)
    with pytest.raises(RuntimeError, match="n_samples"):
        coarse_draw.draw_samples(torch.ones(4, dtype=torch.bool, device=DEV), 0, 0, 0)


def test_the_draw_makes_no_host_synchronisation():
    mask = torch.as_tensor(_masks(70_000)["half"]).to(DEV)
    coarse_draw.draw_samples(mask, 4097, SEED, CALL); torch.cuda.synchronize()          # (warm: code objects, the allocator)
    torch.cuda.set_sync_debug_mode("error")
    try:
        idx, noise, nm = coarse_draw.draw_samples(mask, 4097, SEED, CALL)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(nm) == int(mask.sum())
