"""Weight-only quantisation of linear weights: ``--quantization fp8`` (W8A16, below) and
``--quantization mxfp4`` (W4A16, OCP MXFP4: the second half of this file).

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
QUANTIZATION_METHODS = ("fp8", "mxfp4")


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


# ------------------------------------------------------------------ MXFP4 (--quantization mxfp4)
# OCP MX v1.0, the layout published MXFP4 checkpoints use.  A weight [N, K] becomes
#   codes  uint8 [N, K/2]:  element 2j is the low nibble of byte j, element 2j+1 the high one;
#                           an e2m1 code is sign bit 3 and magnitude bits 2..0;
#   scales uint8 [N, K/32]: e8m0 (biased exponent b, value 2^(b-127)), one per 32 consecutive
#                           k of one row.
# That is 4.25 bits per weight.  The GPU kernels (csrc/kernels/gemm_w4.hip) read this layout
# directly (one copy on the device) and widen with the hardware conversion, which multiplies
# by the power-of-two scale: the operand is the exact dequantised value.  The scales travel
# with the codes as their ``w4_scale`` attribute.
MXFP4_BLOCK = 32
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def mxfp4_exp_range(dtype: torch.dtype) -> tuple[int, int]:
    """Unbiased block exponents for which every dequantised value (0.5 .. 6 times 2^e) is
    exactly representable in ``dtype`` (and, for f16, normal): bf16 / fp32 [-126, 125],
    f16 [-13, 13]."""
    return (-13, 13) if dtype == torch.float16 else (-126, 125)


def quantize_mxfp4(w: torch.Tensor, dtype=None) -> tuple[torch.Tensor, torch.Tensor]:
    """(codes uint8 [N, K/2], scales uint8 [N, K/32]) of a 2-D weight, on w's device.  Per
    32-block: unbiased exponent e = floor(log2(amax)) - 2 (the OCP rule: amax lands in
    [4, 8) before rounding), clamped to ``mxfp4_exp_range(dtype)`` (``dtype``: the dtype the
    weight is dequantised to, w's own by default); elements w / 2^e rounded to nearest-even
    on the e2m1 grid, saturating at +-6.  An all-zero block gets e = 0 and zero codes.
    |w - dq| <= amax(block) / 4 (where e was not clamped)."""
    assert w.dim() == 2 and w.shape[1] % MXFP4_BLOCK == 0, "quantize_mxfp4: [N, K], K % 32 == 0"
    N, K = w.shape
    lo, hi = mxfp4_exp_range(w.dtype if dtype is None else dtype)
    wf = w.detach().float().view(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    amax = wf.abs().amax(dim=2)
    ex = torch.frexp(amax)[1]                       # amax = m * 2^ex, m in [0.5, 1)
    e = torch.where(amax > 0, (ex - 3).clamp(lo, hi), torch.zeros_like(ex))
    a = torch.ldexp(wf.abs(), -e[:, :, None]).clamp_(max=6.0)
    # nearest-even on the grid: spacing 0.5 below 2, 1 below 4, 2 up to 6 (torch.round is
    # half-to-even, and the even multiples are the codes with a zero mantissa bit)
    q = torch.where(a < 2, torch.round(a * 2) * 0.5,
                    torch.where(a < 4, torch.round(a), torch.round(a * 0.5) * 2))
    mag = torch.where(q < 2, q * 2, torch.where(q < 4, q + 2, q * 0.5 + 4)).to(torch.uint8)
    code = (mag | (((wf < 0) & (q > 0)).to(torch.uint8) << 3)).view(N, K)
    codes = (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous()
    scales = (e + 127).to(torch.uint8).contiguous()
    return attach_w4_scale(codes, scales), scales


def attach_w4_scale(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    assert codes.dtype == torch.uint8 and scales.dtype == torch.uint8
    assert codes.dim() == 2 and scales.shape == (codes.shape[0], codes.shape[1] // 16)
    codes.w4_scale = scales  # type: ignore[attr-defined]
    return codes


def is_mxfp4(w: torch.Tensor) -> bool:
    return w.dtype == torch.uint8 and getattr(w, "w4_scale", None) is not None


def w4_scale(w4: torch.Tensor) -> torch.Tensor:
    s = getattr(w4, "w4_scale", None)
    if s is None:
        raise RuntimeError("mxfp4 weight without its block scales (quantize_mxfp4 attaches them)")
    return s


MXFP4_TILE_BYTES = 128 * 32 + 256      # a K9mf tile: 128 rows x 64 k of codes + their scales


def pack_mxfp4_tiles_reference(codes: torch.Tensor, scales: torch.Tensor,
                               silu: bool = False) -> torch.Tensor:
    """The packed layout K9mf (csrc/kernels/gemm_w4_decode.hip) streams, in plain torch on
    the codes' device: uint8 [N/128, K/64, 4352], one tile per (column tile nb, 64-k step kb)
    of codes [N, K/2] and scales [N, K/32].  Tile row r holds weight row ``tile_rows(N,
    silu)[nb, r]`` (as K9mq's tiles: ``silu`` interleaves 16-row groups of gate and up).
    Bytes [0, 4096): 32-byte code rows of four 8-byte chunks; the chunk at position p of tile
    row r is k-chunk q = p ^ (2 * ((r // 8) % 2)): code bytes ``32 kb + 4 q + [0, 4)`` of the
    weight row (k = 64 kb + 8 q + [0, 8)) followed by bytes ``32 kb + 16 + 4 q + [0, 4)``
    (k = 64 kb + 32 + 8 q + [0, 8)) -- the two MFMA k-halves one lane feeds; the XOR makes
    the LDS reads conflict-free.  Bytes [4096, 4352): the step's scales as
    [wn 2][r16 16][n 4][ks 2]: byte ``128 wn + 8 r16 + 2 n + ks`` is scale ``2 kb + ks`` of
    tile row ``64 wn + 16 n + r16``."""
    assert codes.dim() == 2 and codes.dtype == torch.uint8 and scales.dtype == torch.uint8
    N, K = codes.shape[0], 2 * codes.shape[1]
    assert scales.shape == (N, K // MXFP4_BLOCK)
    assert N % 128 == 0 and K % 64 == 0 and (not silu or (N // 2) % 64 == 0)
    dev = codes.device
    nb, nk = N // 128, K // 64
    r = torch.arange(128, device=dev)
    rows = tile_rows(N, silu, dev)
    t = codes.contiguous()[rows]                              # [nb, r, K/2]
    t = t.view(nb, 128, nk, 2, 4, 4)                          # [nb, r, kb, half, q, e]
    t = t.permute(0, 2, 1, 4, 3, 5)                           # [nb, kb, r, q, half, e]
    q = torch.arange(4, device=dev)[None, :] ^ (2 * ((r // 8) % 2))[:, None]
    c = t[:, :, r[:, None], q].reshape(nb, nk, 4096)          # [nb, kb, r, position, half, e]
    s = scales.contiguous()[rows]                             # [nb, r, K/32]
    s = s.view(nb, 2, 4, 16, nk, 2)                           # [nb, wn, n, r16, kb, ks]
    s = s.permute(0, 4, 1, 3, 2, 5).reshape(nb, nk, 256)      # [nb, kb, wn, r16, n, ks]
    return torch.cat([c, s], dim=2).contiguous()


def dequantize_mxfp4(codes: torch.Tensor, scales: torch.Tensor,
                     dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """[N, K] ``dtype`` from codes [N, K/2] and scales [N, K/32], in plain torch: the CPU
    path and the oracle of the GPU kernels.  The fp32 scale is built from the e8m0 byte as
    ``b << 23``, as the kernels build it; value * scale is exact in fp32, and exact in
    ``dtype`` for the exponents ``quantize_mxfp4`` produces for it."""
    N, K = codes.shape[0], codes.shape[1] * 2
    lut = torch.tensor(E2M1_VALUES + tuple(-v for v in E2M1_VALUES), dtype=torch.float32,
                       device=codes.device)
    v = torch.stack([lut[(codes & 0xF).long()], lut[(codes >> 4).long()]], dim=-1)
    sc = (scales.to(torch.int32) << 23).view(torch.float32)
    return (v.view(N, K // MXFP4_BLOCK, MXFP4_BLOCK) * sc[:, :, None]).view(N, K).to(dtype)
