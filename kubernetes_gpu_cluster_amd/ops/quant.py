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


# chunk position XOR of the K9mq weight tiles, by (tile row // 4) % 4
_TILE_SWZ = (0, 2, 3, 1)


def tile_rows(N: int, silu: bool, device=None) -> torch.Tensor:
    """[N/128, 128] int64: the weight row that tile row r of column tile nb holds (see
    ``pack_fp8_tiles_reference``)."""
    r = torch.arange(128, device=device)
    nb = torch.arange(N // 128, device=device)[:, None]
    if silu:
        g = r // 16
        return (g % 2) * (N // 2) + nb * 64 + (g // 2) * 16 + r % 16
    return nb * 128 + r


def pack_fp8_tiles_reference(w8: torch.Tensor, silu: bool = False) -> torch.Tensor:
    """The packed layout K9mq (csrc/kernels/gemm_w8_decode.hip) streams, in plain torch on
    w8's device: uint8 [N/128, K/64, 8192], one 128-row x 64-byte tile per (column tile nb,
    K-step kb).  Tile row r holds weight row ``128 nb + r`` -- or, ``silu`` (a merged
    [gate; up] weight [2I, K]), 16-row groups of gate and up interleaved: group g = r // 16
    is rows ``64 nb + 16 (g // 2) + [0, 16)`` of gate (g even) or of up (g odd, + I).  The
    16-byte chunk at position p of a tile row is k-chunk q = p ^ (0, 2, 3, 1)[(r // 4) % 4]:
    the 8 bytes k = 64 kb + 8 q + [0, 8) followed by the 8 bytes k = 64 kb + 32 + 8 q + [0, 8)
    (the two MFMA k-halves one lane feeds; the XOR makes the LDS reads conflict-free)."""
    assert w8.dim() == 2 and w8.dtype == FP8
    N, K = w8.shape
    assert N % 128 == 0 and K % 64 == 0 and (not silu or (N // 2) % 64 == 0)
    dev = w8.device
    r = torch.arange(128, device=dev)
    rows = tile_rows(N, silu, dev)
    t = w8.contiguous().view(torch.uint8)[rows]               # [nb, r, K]
    t = t.view(N // 128, 128, K // 64, 2, 4, 8)               # [nb, r, kb, half, q, e]
    t = t.permute(0, 2, 1, 4, 3, 5)                           # [nb, kb, r, q, half, e]
    swz = torch.tensor(_TILE_SWZ, device=dev)[(r // 4) % 4]
    q = torch.arange(4, device=dev)[None, :] ^ swz[:, None]   # [r, position] -> k-chunk
    out = t[:, :, r[:, None], q]                              # [nb, kb, r, position, half, e]
    return out.reshape(N // 128, K // 64, 8192).contiguous()
