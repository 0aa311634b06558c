"""Build an ``nn.Module`` whose parameter *names and shapes* equal the reference module's.

The engine models do not execute ``nn.Conv2d``; they only need to own tensors under the checkpoint's key
names so that ``state_dict()``, strict ``load_state_dict()``, ``.to()``, ``.half()`` behave exactly as for
the reference modules (SURVEY.md §8b "What the returned object must support").  ``ParamTree`` is a bare
container node; ``build_param_tree`` nests nodes along the dotted key path.
"""

from __future__ import annotations

import math
from typing import Mapping, Sequence

import torch
from torch import nn


class ParamShapes(dict):
    """``dotted.name -> shape`` of a module's parameters, in registration order (the order of its state_dict)."""

    def conv(self, name: str, co: int, ci: int, k: int) -> None:
        self[f'{name}.weight'] = (co, ci, k, k)
        self[f'{name}.bias'] = (co,)

    def linear(self, name: str, co: int, ci: int, bias: bool = True) -> None:
        self[f'{name}.weight'] = (co, ci)
        if bias:
            self[f'{name}.bias'] = (co,)

    def norm(self, name: str, c: int) -> None:
        self[f'{name}.weight'] = (c,)
        self[f'{name}.bias'] = (c,)

    def pixelshuffle_head(self, cin: int, nf: int, cout: int, upscale: int) -> None:
        """conv_before_upsample -> Upsample (a conv + PixelShuffle per factor 2, or one for 3) -> conv_last."""
        self.conv('conv_before_upsample.0', nf, cin, 3)
        if upscale == 3:
            self.conv('upsample.0', 9 * nf, nf, 3)
        elif upscale & (upscale - 1) == 0:
            for u in range(int(math.log2(upscale))):
                self.conv(f'upsample.{2 * u}', 4 * nf, nf, 3)
        else:
            raise ValueError(f'scale {upscale} is not supported. Supported scales: 2^n and 3.')
        self.conv('conv_last', cout, nf, 3)


class ParamTree(nn.Module):
    """A container node: children are ParamTrees or Parameters/buffers named by one key component."""

    def forward(self, *args, **kwargs):  # pragma: no cover - never executed
        raise RuntimeError('ParamTree only stores parameters; the engine runs the forward pass')


def build_param_tree(root: nn.Module, shapes: Mapping[str, Sequence[int]], buffers: Mapping[str, torch.Tensor] | None = None) -> None:
    """Register an (uninitialised, zero) fp32 Parameter for every ``dotted.name -> shape``."""

    def node_for(path: list[str]) -> nn.Module:
        node = root
        for comp in path:
            child = node._modules.get(comp)
            if child is None:
                child = ParamTree()
                node.add_module(comp, child)
            node = child
        return node

    for name, shape in shapes.items():
        *path, leaf = name.split('.')
        node_for(path).register_parameter(leaf, nn.Parameter(torch.zeros(tuple(shape), dtype=torch.float32), requires_grad=False))
    for name, value in (buffers or {}).items():
        *path, leaf = name.split('.')
        node_for(path).register_buffer(leaf, value.clone())
