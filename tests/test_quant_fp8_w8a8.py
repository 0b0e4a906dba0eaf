"""--quantization fp8_w8a8 without a GPU: the flag, the refusals, and the tiny CPU engine,
whose linears above 64 rows quantise their activations per token (the GPU path's oracle)."""
import argparse

import pytest
import torch
import torch.nn.functional as F

from kubernetes_gpu_cluster_amd.engine.config import EngineConfig, add_engine_args, config_from_args
from kubernetes_gpu_cluster_amd.models.quant import dense_projections
from kubernetes_gpu_cluster_amd.ops import gemm
from kubernetes_gpu_cluster_amd.ops.quant import (FP8, dequantize_fp8_rows, quantize_fp8_rows,
                                                   takes_act_fp8, w8_scale)

METHOD = "fp8_w8a8"


def _parse(*argv):
    return config_from_args(add_engine_args(argparse.ArgumentParser()).parse_args(
        ["--model", "tiny-llama", *argv]))


def _engine(model="tiny-llama", quantization=METHOD):
    from kubernetes_gpu_cluster_amd.engine.llm_engine import LLMEngine
    return LLMEngine(EngineConfig(model=model, random_init=True, device="cpu", dtype="float32",
                                  quantization=quantization, max_model_len=128, max_num_seqs=2,
                                  max_num_batched_tokens=128, num_gpu_blocks_override=32))


@pytest.mark.parametrize("argv", [("--quantization", METHOD), ("--quantization=" + METHOD,),
                                  ("-q", METHOD)])
def test_flag_parses_and_int4_is_still_refused(argv):
    assert _parse(*argv).quantization == METHOD
    with pytest.raises(ValueError, match="quantization"):
        _parse("--quantization", "int4")


@pytest.mark.parametrize("name", ["tiny-mixtral", "tiny-opt"])
def test_moe_and_opt_are_refused(name):
    with pytest.raises(ValueError, match=METHOD):
        _engine(name)


def test_cpu_engine_quantises_activations_above_64_rows():
    from kubernetes_gpu_cluster_amd.engine.sequence import SamplingParams
    eng = _engine()
    model = eng.executor.runner.model
    assert model.quantization == METHOD
    ws = [m.weight for l in model.layers for m in dense_projections(l)]
    assert all(w.dtype == FP8 and takes_act_fp8(w) and w8_scale(w).dtype == torch.float32
               for w in ws)
    g = torch.Generator().manual_seed(0)
    prompt = torch.randint(5, 1000, (70,), generator=g).tolist()
    s = eng.add_request(prompt, SamplingParams(temperature=0.0, max_tokens=3, ignore_eos=True))
    while eng.has_unfinished():
        eng.step()
    assert len(s.output_token_ids) == 3
    # a 70-row linear on the engine's own weight is the activation-quantised formula ...
    w = ws[0]
    wd = dequantize_fp8_rows(w, w8_scale(w))
    x = torch.randn(70, w.shape[1], generator=g) * (2.0 ** (torch.arange(70) % 7))[:, None]
    xq, xs = quantize_fp8_rows(x)
    assert torch.equal(gemm.linear(x, w), F.linear(dequantize_fp8_rows(xq, xs), wd))
    # ... which the fp8 method's output (bf16 activations as they are) differs from ...
    fp8 = _engine(quantization="fp8").executor.runner.model
    w16 = dense_projections(fp8.layers[0])[0].weight
    assert torch.equal(w16.view(torch.uint8), w.view(torch.uint8)) and not takes_act_fp8(w16)
    assert torch.equal(gemm.linear(x, w16), F.linear(x, wd))
    assert not torch.equal(gemm.linear(x, w16), gemm.linear(x, w))
    # ... and at 16 rows (K9q's range on the GPU) the two modes are one
    assert torch.equal(gemm.linear(x[:16], w), gemm.linear(x[:16], w16))
