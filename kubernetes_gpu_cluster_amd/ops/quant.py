"""Weight-only FP8 (W8A16) quantisation of linear weights: ``--quantization fp8``.

A weight [N, K] becomes OCP e4m3 (``torch.float8_e4m3fn``) with one fp32 scale per output
row: ``scale = amax(|row|) / 448``, so each row uses the whole e4m3 range, and
``w ~= w8 * scale[:, None]`` to within 2^-4 * amax(row) elementwise (3 mantissa bits).
Activations stay bf16 / f16: the GPU kernels (csrc/kernels/gemm_w8.hip) widen the e4m3
values exactly and apply the scale to the fp32 sums.

The scale travels with the weight tensor as its ``w8_scale`` attribute, because the model
code passes ``layer.weight`` around bare (ops/gemm.py reads it back with ``w8_scale``).
"""
from __future__ import annotations

import torch

FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0
QUANTIZATION_METHODS = ("fp8",)


def quantize_fp8_rows(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """(w8 [N, K] float8_e4m3fn, scale [N] float32) of a 2-D weight, on w's device.  An
    all-zero row gets scale 1; values are clamped to +-448 before the cast (e4m3fn has no
    inf, and an overflowing cast would give NaN)."""
    assert w.dim() == 2, "quantize_fp8_rows: [N, K] weight"
    wf = w.detach().float()
    amax = wf.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax))
    w8 = (wf / scale[:, None]).clamp_(-FP8_MAX, FP8_MAX).to(FP8)
    return attach_scale(w8, scale), scale


def attach_scale(w8: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    assert w8.dtype == FP8 and scale.dtype == torch.float32 and scale.shape == w8.shape[:1]
    w8.w8_scale = scale  # type: ignore[attr-defined]
    return w8


def is_fp8(w: torch.Tensor) -> bool:
    return w.dtype == FP8


def w8_scale(w8: torch.Tensor) -> torch.Tensor:
    s = getattr(w8, "w8_scale", None)
    if s is None:
        raise RuntimeError("fp8 weight without its row scales (quantize_fp8_rows attaches them)")
    return s


def dequantize_fp8_rows(w8: torch.Tensor, scale: torch.Tensor,
                        dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """w8 * scale[:, None], computed in fp32 and rounded once to ``dtype``."""
    return (w8.float() * scale[:, None]).to(dtype)
