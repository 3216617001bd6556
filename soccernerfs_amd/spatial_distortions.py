"""SceneContraction of NS/field_components/spatial_distortions.py:42-89 (positions only; the Gaussian branch belongs to mip-NeRF-style
fields, which this path does not have): f(x) = x for ||x|| < 1, (2 - 1/||x||) x/||x|| otherwise; order = inf contracts onto the cube
[-2, 2]^3, which the K-Planes fields then halve into grid_sample's [-1, 1] (NS/fields/kplanes_field.py:278-280, :438-440).
This module is the elementwise torch form.  For order = inf the K-Planes kernels evaluate the same float32 expression, operation by operation,
where they derive a sample's coordinate from its ray (snerf_coords.contract = 1): the fields with compact ray samples, the
fused trainer and the renderer (bounded = False) take that route and never materialise positions.  Any other order, and explicit positions
(density_fn), run through this module in front of a gather of explicit points."""
from typing import Optional, Union

import torch
from torch import nn


class SpatialDistortion(nn.Module):
    """spatial_distortions.py:27-39."""

    def forward(self, positions: torch.Tensor) -> torch.Tensor:  # pragma: no cover - interface
        raise NotImplementedError


class SceneContraction(SpatialDistortion):
    def __init__(self, order: Optional[Union[float, int]] = None) -> None:
        super().__init__()
        self.order = order

    def forward(self, positions: torch.Tensor) -> torch.Tensor:
        mag = torch.linalg.norm(positions, ord=self.order, dim=-1)[..., None]
        return torch.where(mag < 1, positions, (2 - (1 / mag)) * (positions / mag))
