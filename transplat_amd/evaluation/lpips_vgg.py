"""The weights of LPIPS(net="vgg"), version 0.1: VGG16's thirteen 3x3 convolutions and the five learned
1x1 tap weights (reference src/evaluation/metrics.py:22-33 builds the metric with the `lpips` package,
which downloads both on first use; here they are read from files the user supplies)."""
from __future__ import annotations

from typing import Mapping, Optional

import torch

# (c_in, c_out) of the thirteen convolutions, and their indices in torchvision's vgg16().features
VGG_CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512),
                (512, 512), (512, 512), (512, 512), (512, 512))
VGG_FEATURES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
VGG_BLOCKS = (2, 2, 3, 3, 3)  # convolutions per block; a tap after each block, a 2x2 max-pool between blocks
TAP_CHANNELS = (64, 128, 256, 512, 512)  # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
MIN_SIZE = 16  # below it the fourth pool leaves an empty map


def _slice_of(conv: int) -> int:
    """The lpips package's `net.slice{1..5}` that holds convolution `conv` (0..12)."""
    done = 0
    for k, count in enumerate(VGG_BLOCKS):
        done += count
        if conv < done:
            return k + 1
    raise IndexError(conv)


def _take(sd: Mapping[str, torch.Tensor], key: str, shape: tuple) -> torch.Tensor:
    if key not in sd:
        raise KeyError(f"LpipsVGG: missing key {key!r}")
    t = sd[key]
    if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape):
        got = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"LpipsVGG: {key!r} is {got}, expected {tuple(shape)}")
    return t.detach().to(torch.float32).contiguous()


class LpipsVGG:
    """`convs`: 13 (weight [c_out, c_in, 3, 3], bias [c_out]) fp32 pairs in network order; `lins`: the 5
    tap weight vectors [C] fp32 (non-negative, no bias)."""

    def __init__(self, convs, lins):
        self.convs = [(w, b) for w, b in convs]
        self.lins = list(lins)
        if len(self.convs) != len(VGG_CHANNELS) or len(self.lins) != len(TAP_CHANNELS):
            raise ValueError(f"LpipsVGG: {len(self.convs)} convolutions and {len(self.lins)} taps, expected 13 and 5")
        for i, ((w, b), (ci, co)) in enumerate(zip(self.convs, VGG_CHANNELS)):
            if tuple(w.shape) != (co, ci, 3, 3) or tuple(b.shape) != (co,):
                raise ValueError(f"LpipsVGG: convolution {i} is {tuple(w.shape)} / {tuple(b.shape)}, expected "
                                 f"{(co, ci, 3, 3)} / {(co,)}")
        for k, (v, c) in enumerate(zip(self.lins, TAP_CHANNELS)):
            if tuple(v.shape) != (c,):
                raise ValueError(f"LpipsVGG: tap {k} weights are {tuple(v.shape)}, expected {(c,)}")

    @property
    def device(self) -> torch.device:
        return self.convs[0][0].device

    def tensors(self) -> list[torch.Tensor]:
        return [t for pair in self.convs for t in pair] + self.lins

    def to(self, device) -> "LpipsVGG":
        """The same weights on `device` (self when they are there already). The Winograd-transformed
        filters are cached per weight tensor by kernels.wino_pack_weight, so keep the moved object."""
        device = torch.device(device)
        if all(t.device == device for t in self.tensors()):
            return self
        return LpipsVGG([(w.to(device), b.to(device)) for w, b in self.convs], [v.to(device) for v in self.lins])

    @classmethod
    def from_state_dict(cls, sd: Mapping[str, torch.Tensor], lin_sd: Optional[Mapping[str, torch.Tensor]] = None):
        """Layout (a), `lin_sd` None: the whole metric's state dict, `net.slice{1..5}.{i}.weight|bias` with i
        the VGG16 `features` index and `lin{0..4}.model.1.weight` [1, C, 1, 1]. Layout (b): a torchvision
        VGG16 state dict (`features.{i}.weight|bias`, other keys ignored) and `lin_sd` with the
        `lin{k}.model.1.weight` keys. A missing key raises KeyError, a mis-shaped one ValueError, both
        naming the key; a `scaling_layer.shift|scale` entry that is not the metric's constants raises."""
        for src in (sd, lin_sd or {}):
            for name, want in (("shift", SHIFT), ("scale", SCALE)):
                key = f"scaling_layer.{name}"
                if key in src:
                    got = src[key].detach().double().flatten()
                    if got.numel() != 3 or (got - torch.tensor(want, dtype=torch.float64)).abs().max() > 1e-6:
                        raise ValueError(f"LpipsVGG: {key!r} is {got.tolist()}, this metric is defined with {want}")
        convs = []
        for n, (idx, (ci, co)) in enumerate(zip(VGG_FEATURES, VGG_CHANNELS)):
            stem = f"features.{idx}" if lin_sd is not None else f"net.slice{_slice_of(n)}.{idx}"
            convs.append((_take(sd, f"{stem}.weight", (co, ci, 3, 3)), _take(sd, f"{stem}.bias", (co,))))
        lin_src = lin_sd if lin_sd is not None else sd
        lins = [_take(lin_src, f"lin{k}.model.1.weight", (1, c, 1, 1)).reshape(c) for k, c in enumerate(TAP_CHANNELS)]
        return cls(convs, lins)

    @classmethod
    def from_files(cls, path, lin_path=None):
        """`path` alone: layout (a); with `lin_path`: layout (b) (see from_state_dict). Both files are read
        with torch.load(weights_only=True, map_location="cpu")."""
        sd = torch.load(path, weights_only=True, map_location="cpu")
        lin_sd = torch.load(lin_path, weights_only=True, map_location="cpu") if lin_path is not None else None
        return cls.from_state_dict(sd, lin_sd)

    @classmethod
    def seeded(cls, seed: int = 0):
        """Random weights of the right shapes for tests and timing only: NOT a metric, its values mean
        nothing perceptually. Convolution weights N(0, 2 / (9 c_in)), biases N(0, 0.05^2), tap weights
        U[0, 1) / C, drawn from one torch.Generator in float64 in layer order (weight, bias per
        convolution, then the five taps) and rounded to fp32."""
        gen = torch.Generator().manual_seed(seed)
        convs = []
        for ci, co in VGG_CHANNELS:
            w = torch.randn((co, ci, 3, 3), generator=gen, dtype=torch.float64) * (2.0 / (9 * ci)) ** 0.5
            b = torch.randn((co,), generator=gen, dtype=torch.float64) * 0.05
            convs.append((w.float(), b.float()))
        lins = [(torch.rand((c,), generator=gen, dtype=torch.float64) / c).float() for c in TAP_CHANNELS]
        return cls(convs, lins)
