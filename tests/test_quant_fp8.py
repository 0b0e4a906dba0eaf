"""``--quantization fp8`` (weight-only W8A16) on the CPU: the row quantiser, the flag, and
engine parity of a quantised model against HF loaded with the dequantised weights."""
import argparse

import pytest
import torch

from kubernetes_gpu_cluster_amd.engine.config import EngineConfig, add_engine_args, config_from_args
from kubernetes_gpu_cluster_amd.models import PRESETS, build_model, full_state_dict_random
from kubernetes_gpu_cluster_amd.models.quant import dense_projections, quantize_model
from kubernetes_gpu_cluster_amd.ops.quant import (dequantize_fp8_rows, quantize_fp8_rows,
                                                  w8_scale)
from kubernetes_gpu_cluster_amd.parallel.state import ParallelState, set_state

FP8 = torch.float8_e4m3fn


# ------------------------------------------------------------------ quantiser
def _rows():
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(48, 320, generator=g) * 0.05).to(torch.bfloat16)
    w[5] = 0                                   # an all-zero row
    w[7] *= 2.0 ** 9                           # rows of very different magnitude
    w[9] *= 2.0 ** -9
    return w


def test_quantizer_dtypes_and_zero_row():
    w = _rows()
    w8, scale = quantize_fp8_rows(w)
    assert w8.dtype == FP8 and w8.shape == w.shape
    assert scale.dtype == torch.float32 and scale.shape == (w.shape[0],)
    assert scale[5].item() == 1.0
    assert torch.isfinite(w8.float()).all() and torch.isfinite(scale).all()
    assert (w8.float()[5] == 0).all()
    assert w8_scale(w8) is scale               # the scale travels with the weight
    amax = w.float().abs().amax(1)
    torch.testing.assert_close(scale[amax > 0], (amax / 448)[amax > 0], rtol=1e-6, atol=0)
    assert w8.float().abs().max().item() <= 448.0


def test_quantizer_error_within_format_bound():
    """|w - w8 * scale| <= 2^-4 * amax(row): 3 mantissa bits, amax mapped to 448."""
    w = _rows()
    w8, scale = quantize_fp8_rows(w)
    err = (w.float() - dequantize_fp8_rows(w8, scale)).abs()
    bound = 2.0 ** -4 * w.float().abs().amax(1, keepdim=True)
    print("worst error / bound:", (err / bound.clamp_min(1e-30)).max().item())
    assert bool((err <= bound).all())


def test_quantizer_clamps_before_cast():
    """A value that would land just above 448 after the division is clamped, not NaN."""
    w = torch.tensor([[1.0, -1.0, 0.5, 3.0e38], [float(2 ** -140), 0.0, 0.0, 0.0]])
    w8, scale = quantize_fp8_rows(w)
    assert torch.isfinite(w8.float()).all() and torch.isfinite(scale).all()


def test_every_e4m3_code_widens_exactly():
    """Every finite e4m3 code is a bf16 and an f16 value: the kernels' widening is exact."""
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(FP8)
    f = codes.float()
    finite = torch.isfinite(f)
    assert int(finite.sum()) == 254            # e4m3fn: only the two NaN codes are not finite
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal(f[finite].to(dt).float(), f[finite])


# ------------------------------------------------------------------ flags
def _parse(*argv):
    return config_from_args(add_engine_args(argparse.ArgumentParser()).parse_args(
        ["--model", "tiny-llama", *argv]))


def test_flag_parses_both_spellings_and_defaults_to_none():
    assert _parse("--quantization", "fp8").quantization == "fp8"
    assert _parse("--quantization=fp8").quantization == "fp8"
    assert _parse().quantization is None
    assert EngineConfig().quantization is None


def test_flag_rejects_other_methods():
    with pytest.raises(ValueError, match="quantization"):
        _parse("--quantization", "int4")


@pytest.mark.parametrize("name", ["tiny-mixtral", "tiny-opt"])
def test_out_of_scope_models_raise_at_setup(name):
    from kubernetes_gpu_cluster_amd.engine.llm_engine import LLMEngine
    with pytest.raises(ValueError, match="quantization"):
        LLMEngine(EngineConfig(model=name, random_init=True, device="cpu", quantization="fp8",
                               max_model_len=64, max_num_seqs=2, max_num_batched_tokens=64,
                               num_gpu_blocks_override=16))


def test_engine_generates_with_the_flag_on_cpu():
    from kubernetes_gpu_cluster_amd.engine.llm_engine import LLMEngine
    from kubernetes_gpu_cluster_amd.engine.sequence import SamplingParams
    eng = LLMEngine(EngineConfig(model="tiny-llama", random_init=True, device="cpu",
                                 dtype="float32", quantization="fp8", max_model_len=64,
                                 max_num_seqs=2, max_num_batched_tokens=64,
                                 num_gpu_blocks_override=16))
    model = eng.executor.runner.model
    assert model.quantization == "fp8"
    assert all(m.weight.dtype == FP8 for l in model.layers for m in dense_projections(l))
    s = eng.add_request([5, 9, 13], SamplingParams(temperature=0.0, max_tokens=3, ignore_eos=True))
    while eng.has_unfinished():
        eng.step()
    assert len(s.output_token_ids) == 3


# ------------------------------------------------------------------ engine parity on CPU
@pytest.mark.parametrize("name", ["tiny-llama", "tiny-qwen2"])
def test_quantized_logits_match_hf_on_dequantized_weights(name):
    pytest.importorskip("transformers")
    from test_model_parity import _engine_logits, _hf_model, _ours
    cfg = PRESETS[name]
    sd = full_state_dict_random(cfg, seed=1, std=0.05)
    model, runner = _ours(cfg, sd)
    bf16_bytes = {}
    for i, l in enumerate(model.layers):
        for j, m in enumerate(dense_projections(l)):
            bf16_bytes[(i, j)] = m.weight.numel() * 2        # what a bf16 build holds
    quantize_model(model)
    assert model.quantization == "fp8"
    assert model.fold_rs_weights() == 0 and not model._fusable
    assert not model.silu_weights() and not model.silu_shapes() and not model.tail_shapes()
    assert not model.fused_norm_shapes() and not model.qkv_dims()
    # the four projections of every layer hold fp8: half the bf16 bytes + 4 N of scales
    for i, l in enumerate(model.layers):
        for j, m in enumerate(dense_projections(l)):
            w, s = m.weight, w8_scale(m.weight)
            assert w.dtype == FP8 and s.dtype == torch.float32 and s.shape == (w.shape[0],)
            got = w.numel() * w.element_size() + s.numel() * s.element_size()
            assert got == bf16_bytes[(i, j)] // 2 + 4 * w.shape[0]
    assert model.embed_tokens.weight.dtype == torch.float32
    assert model.lm_head.get_weight().dtype == torch.float32
    # HF on the dequantised weights (the merged qkv / gate_up rows split back by name)
    sd_q = dict(sd)
    H, d = cfg.hidden_size, cfg.head_dim
    nq, nkv, I = cfg.num_heads * d, cfg.num_kv_heads * d, cfg.intermediate_size
    for i, l in enumerate(model.layers):
        qkv, o, gu, dn = [dequantize_fp8_rows(m.weight, w8_scale(m.weight))
                          for m in dense_projections(l)]
        p = f"model.layers.{i}."
        sd_q[p + "self_attn.q_proj.weight"] = qkv[:nq]
        sd_q[p + "self_attn.k_proj.weight"] = qkv[nq:nq + nkv]
        sd_q[p + "self_attn.v_proj.weight"] = qkv[nq + nkv:]
        sd_q[p + "self_attn.o_proj.weight"] = o
        sd_q[p + "mlp.gate_proj.weight"] = gu[:I]
        sd_q[p + "mlp.up_proj.weight"] = gu[I:]
        sd_q[p + "mlp.down_proj.weight"] = dn
        for k in ("self_attn.q_proj", "self_attn.o_proj", "mlp.down_proj"):
            assert sd_q[p + k + ".weight"].shape == sd[p + k + ".weight"].shape
            assert not torch.equal(sd_q[p + k + ".weight"], sd[p + k + ".weight"])
    hf, _ = _hf_model(cfg, sd_q)
    g = torch.Generator().manual_seed(0)
    prompt = torch.randint(3, cfg.vocab_size, (37,), generator=g).tolist()
    extra = torch.randint(3, cfg.vocab_size, (5,), generator=g).tolist()
    with torch.no_grad():
        ref = hf(torch.tensor([prompt + extra])).logits[0].float()
    got = _engine_logits(model, runner, prompt, [16, 21], extra)   # chunked prefill + 5 decodes
    torch.testing.assert_close(got, ref[: len(prompt) + len(extra)], atol=2e-4, rtol=2e-4)
