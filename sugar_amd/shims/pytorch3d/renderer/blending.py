"""`pytorch3d.renderer.blending`: `BlendParams` and `softmax_rgb_blend`, restated from pytorch3d 0.7.4's published
`pytorch3d/renderer/blending.py` (operation for operation, so that a CPU run reproduces its rounding).  pytorch3d is not
installed here: PARITY-UNPINNED against pytorch3d itself.  Reached from the texture baking of the refined mesh
(sugar_scene/sugar_model.py:2610-2661, through SoftPhongShader)."""
from __future__ import annotations

from typing import NamedTuple, Sequence, Union

import torch


class BlendParams(NamedTuple):
    sigma: float = 1e-4
    gamma: float = 1e-4
    background_color: Union[torch.Tensor, Sequence[float]] = (1.0, 1.0, 1.0)


def softmax_rgb_blend(colors: torch.Tensor, fragments, blend_params: BlendParams, znear: Union[float, torch.Tensor] = 1.0,
                      zfar: Union[float, torch.Tensor] = 100) -> torch.Tensor:
    """colors (N, H, W, K, 3) of the K faces per pixel -> (N, H, W, 4) RGBA: a softmax over the faces' inverse depths weighted by
    their coverage probability, plus a background term.  A covered pixel beyond zfar gets a negative inverse depth: the
    background term then dominates and the pixel blends towards the background colour."""
    N, H, W, K = fragments.pix_to_face.shape
    device = fragments.pix_to_face.device
    pixel_colors = torch.ones((N, H, W, 4), dtype=colors.dtype, device=colors.device)
    background_ = blend_params.background_color
    if not isinstance(background_, torch.Tensor):
        background = torch.tensor(background_, dtype=torch.float32, device=device)
    else:
        background = background_.to(device)

    eps = 1e-10
    mask = fragments.pix_to_face >= 0
    prob_map = torch.sigmoid(-fragments.dists / blend_params.sigma) * mask
    alpha = torch.prod((1.0 - prob_map), dim=-1)

    if torch.is_tensor(zfar):
        zfar = zfar[:, None, None, None]
    if torch.is_tensor(znear):
        znear = znear[:, None, None, None]

    z_inv = (zfar - fragments.zbuf) / (zfar - znear) * mask
    z_inv_max = torch.max(z_inv, dim=-1).values[..., None].clamp(min=eps)
    weights_num = prob_map * torch.exp((z_inv - z_inv_max) / blend_params.gamma)
    delta = torch.exp((eps - z_inv_max) / blend_params.gamma).clamp(min=eps)
    denom = weights_num.sum(dim=-1)[..., None] + delta

    weighted_colors = (weights_num[..., None] * colors).sum(dim=-2)
    weighted_background = delta * background
    pixel_colors[..., :3] = (weighted_colors + weighted_background) / denom
    pixel_colors[..., 3] = 1.0 - alpha
    return pixel_colors
