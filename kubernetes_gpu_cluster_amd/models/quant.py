"""``--quantization fp8 | mxfp4``: online weight-only quantisation (W8A16 / W4A16) of the
dense Llama-family linears.

After a rank has loaded its shard, the qkv / o / gate_up / down projection weights of every
layer are replaced by their e4m3 form with one fp32 scale per output row, or by their MXFP4
form (e2m1 codes, one e8m0 scale per 32 k of a row) (ops/quant.py); activations, embeddings,
the LM head and the norms keep the model dtype.  Each rank quantises what it holds (MXFP4
blocks lie along K, and a row-parallel shard starts at a multiple of 32), so TP and PP need
nothing extra.
"""
from __future__ import annotations

import logging
from typing import Optional

import torch
import torch.nn as nn

from ..ops.quant import (MXFP4_BLOCK, QUANTIZATION_METHODS, attach_scale, attach_w4_scale, is_fp8,
                         is_mxfp4, quantize_fp8_rows, quantize_mxfp4)
from .configs import ModelConfig

log = logging.getLogger("kgc.quant")


def check_quantizable(cfg: ModelConfig, method: Optional[str]) -> None:
    """Raise ValueError for a method or architecture ``--quantization`` does not cover."""
    if method is None:
        return
    if method not in QUANTIZATION_METHODS:
        raise ValueError(f"--quantization {method} is not supported "
                         f"({'/'.join(QUANTIZATION_METHODS)})")
    if cfg.is_moe:
        raise ValueError(f"--quantization {method}: MoE model {cfg.name!r} is not supported "
                         f"(expert weights run through the grouped expert GEMMs, which take "
                         f"bf16 / f16 only)")
    if cfg.arch == "opt":
        raise ValueError(f"--quantization {method}: OPT model {cfg.name!r} is not supported "
                         f"(LayerNorm, fp16 and biased linears throughout)")


def dense_projections(layer) -> list:
    """The four quantised linears of a dense decoder layer."""
    return [layer.self_attn.qkv_proj, layer.self_attn.o_proj, layer.mlp.gate_up_proj,
            layer.mlp.down_proj]


@torch.no_grad()
def quantize_model(model: nn.Module, method: str = "fp8") -> int:
    """Replace each dense projection weight of ``model`` by its fp8 or mxfp4 form, layer by
    layer (the bf16 copy of a layer is freed before the next is quantised), reserve the widen
    path's scratch and empty the allocator cache so the KV pool sees the saving.  Call after
    the weights are loaded and before anything is packed or folded.  Returns the bytes saved.
    An mxfp4 weight is stored as [N, K/2] bytes: K is the layer's, never ``weight.shape[1]``."""
    check_quantizable(model.cfg, method)
    from ..ops import gemm
    w4 = method == "mxfp4"
    if w4:
        for i, layer in enumerate(model.layers):
            for lin in dense_projections(layer):
                w = lin.weight
                if not is_mxfp4(w) and w.shape[1] % MXFP4_BLOCK:
                    raise ValueError(f"--quantization mxfp4: layer {i} has a projection with "
                                     f"K = {w.shape[1]} on this rank, not a multiple of "
                                     f"{MXFP4_BLOCK} (one scale covers 32 consecutive k)")
    saved, largest, dev = 0, 0, None
    for layer in model.layers:
        for lin in dense_projections(layer):
            w = lin.weight
            if is_fp8(w) or is_mxfp4(w):
                continue
            loader = getattr(w, "weight_loader", None)
            if w4:
                w8, scale = quantize_mxfp4(w.data, model.dtype)
                p = nn.Parameter(w8, requires_grad=False)
                attach_w4_scale(p, scale)
            else:
                w8, scale = quantize_fp8_rows(w.data)
                p = nn.Parameter(w8, requires_grad=False)
                attach_scale(p, scale)
            if loader is not None:
                p.weight_loader = loader  # type: ignore[attr-defined]
            saved += (w.numel() * w.element_size() - w8.numel()
                      - scale.numel() * scale.element_size())
            largest, dev = max(largest, w.numel()), w.device
            lin.weight = p
            del w, w8, scale
    model.quantization = method
    if dev is not None and dev.type == "cuda":
        gemm.w8_reserve(dev, largest, model.dtype)
        torch.cuda.empty_cache()
    log.info("quantization %s: %d layers, %.2f GB of weights saved", method, len(model.layers),
             saved / 1e9)
    return saved
