"""Host side of the coarse stage's default sample draws (csrc/coarse_draw.hip; C ABI: sgr_draw_samples): what
`SuGaR.sample_points_in_gaussians(mask=..., probabilities_proportional_to_volume=False)` draws before its arithmetic
(sugar_model.py:900-923 and the `randn_like` of :926) -- one Gaussian per sample, uniform among the masked ones, and three standard
normals -- without `torch.multinomial`, without the boolean-mask index composition and without its host wait.

The stream is a counter-based one, stated in include/sugar_raster.h and restated in tests/coarse_draw_restatement.py: Philox4x32-10
keyed by `seed`, the counters made of the sample's number and `call`.  The same (mask, n_samples, seed, call) gives the same bits on
every run; the caller advances `call` once per draw.  Weighted draws (`proportional_to_volume`, `_to_opacity`) are not built here:
they stay on the torch statements of `sugar_patch.sample_points_in_gaussians`.

GPU tensors only; the HIP library must be built."""
from __future__ import annotations

import torch

from . import _lib
from ._call import call, need_gpu, ptr

_U64 = (1 << 64) - 1


def draw_samples(mask, n_samples: int, seed: int, call_index: int):
    """(sample_idx int64[N], noise float32[N,3], n_masked int64 0-dim), all on the mask's device: `sample_idx[n]` is one of the rows
    where `mask` (bool [P], P < 2^31) is set, uniformly, and `noise` is standard normal.  No host synchronisation.  When no row is
    set, `n_masked` is 0 and both outputs are zero: the caller decides what to do (the trainer skips the regulariser)."""
    need_gpu("draw_samples", mask=mask)
    if mask.dtype != torch.bool or mask.dim() != 1:
        raise RuntimeError(f"draw_samples: mask must be a bool [P] tensor, got {mask.dtype} {tuple(mask.shape)}")
    P, N, dev = mask.shape[0], int(n_samples), mask.device
    if not 1 <= P < 2 ** 31:
        raise RuntimeError("draw_samples: P must lie in [1, 2^31)")
    if not 1 <= N < 2 ** 32:
        raise RuntimeError("draw_samples: n_samples must lie in [1, 2^32)")
    m = mask.contiguous()
    sample_idx = torch.empty(N, dtype=torch.int64, device=dev)
    noise = torch.empty(N, 3, device=dev)
    n_masked = torch.empty((), dtype=torch.int64, device=dev)
    scratch = torch.empty(_lib.load().sgr_draw_samples_scratch_bytes(P), dtype=torch.uint8, device=dev)
    call("sgr_draw_samples", dev, P, ptr(m), N, int(seed) & _U64, int(call_index) & _U64, ptr(sample_idx), ptr(noise), ptr(n_masked),
         ptr(scratch))
    return sample_idx, noise, n_masked
