"""`pytorch3d.renderer.lighting.AmbientLights` (pytorch3d 0.7.4): uniform ambient light, no diffuse or specular term.  The only
light the stand-in shader supports (sugar_scene/sugar_model.py:2615); PARITY-UNPINNED against pytorch3d itself."""
from __future__ import annotations

import torch


class AmbientLights:
    def __init__(self, ambient_color=None, device="cpu"):
        if ambient_color is None:
            ambient_color = ((1.0, 1.0, 1.0),)
        c = torch.as_tensor(ambient_color, dtype=torch.float32, device=device)
        self.ambient_color = c[None] if c.dim() == 1 else c
        self.device = torch.device(device)

    def to(self, device):
        self.ambient_color = self.ambient_color.to(device)
        self.device = torch.device(device)
        return self

    def diffuse(self, normals, points=None):
        return torch.zeros_like(points if points is not None else normals)

    def specular(self, normals, points, camera_position, shininess):
        return torch.zeros_like(points)
