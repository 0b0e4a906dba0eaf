"""``--quantization mxfp4`` (weight-only W4A16, OCP MXFP4) on the CPU: the block quantiser and
its plain-torch inverse, the flag, and engine parity of a quantised model against HF loaded
with the dequantised weights."""
import argparse

import pytest
import torch

from kubernetes_gpu_cluster_amd.engine.config import EngineConfig, add_engine_args, config_from_args
from kubernetes_gpu_cluster_amd.models import PRESETS, full_state_dict_random
from kubernetes_gpu_cluster_amd.models.quant import dense_projections, quantize_model
from kubernetes_gpu_cluster_amd.ops.quant import (E2M1_VALUES, dequantize_mxfp4, is_mxfp4,
                                                  mxfp4_exp_range, quantize_mxfp4, w4_scale)


# ------------------------------------------------------------------ flags
def _parse(*argv):
    return config_from_args(add_engine_args(argparse.ArgumentParser()).parse_args(
        ["--model", "tiny-llama", *argv]))


def test_flag_parses_both_spellings():
    assert _parse("--quantization", "mxfp4").quantization == "mxfp4"
    assert _parse("--quantization=mxfp4").quantization == "mxfp4"
    assert _parse("-q", "mxfp4").quantization == "mxfp4"
    assert EngineConfig(quantization="mxfp4").quantization == "mxfp4"
    with pytest.raises(ValueError, match="quantization"):
        _parse("--quantization", "int4")


@pytest.mark.parametrize("name", ["tiny-mixtral", "tiny-opt"])
def test_out_of_scope_models_raise_at_setup(name):
    from kubernetes_gpu_cluster_amd.engine.llm_engine import LLMEngine
    with pytest.raises(ValueError, match="quantization mxfp4"):
        LLMEngine(EngineConfig(model=name, random_init=True, device="cpu", quantization="mxfp4",
                               max_model_len=64, max_num_seqs=2, max_num_batched_tokens=64,
                               num_gpu_blocks_override=16))


# ------------------------------------------------------------------ quantiser
def _rows():
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(48, 320, generator=g) * 0.05).to(torch.bfloat16)
    w[5] = 0                                   # a row of all-zero blocks
    w[6, 64:96] = 0                            # one zero block inside a row
    w[7] *= 2.0 ** 9                           # rows of very different magnitude
    w[9] *= 2.0 ** -9
    return w


def test_quantizer_shapes_codes_and_zero_blocks():
    w = _rows()
    N, K = w.shape
    codes, scales = quantize_mxfp4(w)
    assert codes.dtype == torch.uint8 and codes.shape == (N, K // 2) and codes.is_contiguous()
    assert scales.dtype == torch.uint8 and scales.shape == (N, K // 32) and scales.is_contiguous()
    assert codes.numel() * codes.element_size() + scales.numel() == N * K // 2 + N * K // 32
    assert is_mxfp4(codes) and w4_scale(codes) is scales     # the scales travel with the codes
    assert not is_mxfp4(torch.zeros(2, 16, dtype=torch.uint8))
    # an all-zero block: e = 0 (byte 127) and zero codes
    assert bool((scales[5] == 127).all()) and bool((codes[5] == 0).all())
    assert scales[6, 2].item() == 127 and bool((codes[6, 32:48] == 0).all())
    assert bool((scales != 0xFF).all())                      # the e8m0 NaN code
    # a block's largest element lands on 4 or 6 (amax / 2^e is in [4, 8))
    dq = dequantize_mxfp4(codes, scales).view(N, K // 32, 32)
    e = scales.float() - 127
    top = dq.abs().amax(2) / 2.0 ** e
    nz = w.float().view(N, K // 32, 32).abs().amax(2) > 0
    assert bool(((top == 4) | (top == 6))[nz].all())
    # element 2j is the low nibble of byte j, element 2j + 1 the high one
    one = torch.zeros(1, 32)
    one[0, 0], one[0, 1], one[0, 31] = 1.0, -3.0, 6.0
    c1, s1 = quantize_mxfp4(one)
    assert s1.item() == 127 and c1[0, 0].item() == (2 | (0x8 | 5) << 4) and c1[0, 15].item() == 7 << 4


def test_quantizer_error_within_format_bound():
    """|w - dq| <= amax(block) / 4: grid spacing at most 2 * 2^e with 2^e <= amax / 4, and a
    saturated element is off by v - 6 * 2^e < amax / 4."""
    w = _rows()
    codes, scales = quantize_mxfp4(w)
    wf = w.float().view(48, 10, 32)
    err = (wf - dequantize_mxfp4(codes, scales).view(48, 10, 32)).abs()
    bound = wf.abs().amax(2, keepdim=True) / 4
    print("worst error / bound:", (err / bound.clamp_min(1e-30)).max().item())
    assert bool((err <= bound).all())
    assert scales[7].float().mean() > scales[9].float().mean() + 16     # 2^9 against 2^-9


def test_round_to_nearest_even_and_saturation():
    """Ties go to the code with an even mantissa bit; beyond 6 saturates."""
    v = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 5.1, 7.9, -0.25, -2.5, -7.0, 4.0]
    exp = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 6.0, 6.0, 0.0, -2.0, -6.0, 4.0]
    w = torch.zeros(1, 32)
    w[0, :len(v)] = torch.tensor(v)          # amax 7.9: e = 0
    codes, scales = quantize_mxfp4(w)
    assert scales[0, 0].item() == 127
    assert dequantize_mxfp4(codes, scales)[0, :len(v)].tolist() == exp


def test_every_code_and_exponent_dequantises_exactly():
    """Every (code, in-range exponent) pair is a bf16 value, and an f16 value in f16's range:
    the kernels' widening is exact."""
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(16, 16)
    for dt in (torch.bfloat16, torch.float16):
        lo, hi = mxfp4_exp_range(dt)
        for e in range(lo, hi + 1):
            sc = torch.full((16, 1), e + 127, dtype=torch.uint8)
            f = dequantize_mxfp4(codes, sc)                       # fp32, exact by construction
            lut = torch.tensor(E2M1_VALUES + tuple(-x for x in E2M1_VALUES), dtype=torch.float64)
            want = torch.stack([lut[(codes & 15).long()], lut[(codes >> 4).long()]], -1)
            assert torch.equal(f.double().view(16, 16, 2), want * 2.0 ** e)
            assert torch.isfinite(f).all()
            assert torch.equal(f.to(dt).float(), f), (dt, e)
            assert torch.equal(dequantize_mxfp4(codes, sc, dt).float(), f)


def test_f16_exponent_clamp():
    """Blocks with amax 2^-30 and 2^20 keep finite f16 values, every non-zero one normal."""
    w = torch.zeros(2, 64, dtype=torch.float32)
    w[0, :32] = 2.0 ** -30
    w[0, 32:] = torch.linspace(-1, 1, 32) * 2.0 ** -12
    w[1] = torch.linspace(-1, 1, 64) * 2.0 ** 20
    codes, scales = quantize_mxfp4(w, torch.float16)       # fp32 weights of an f16 model
    lo, hi = mxfp4_exp_range(torch.float16)
    assert (lo, hi) == (-13, 13)
    assert int(scales.min()) >= lo + 127 and int(scales.max()) <= hi + 127
    dq = dequantize_mxfp4(codes, scales, torch.float16)
    assert torch.isfinite(dq).all()
    nzv = dq[dq != 0].float().abs()
    assert nzv.numel() and nzv.min().item() >= 2.0 ** -14            # f16's smallest normal
    assert dq.float().abs().max().item() == 6 * 2.0 ** 13
    # the same weights as bf16 are not clamped
    c2, s2 = quantize_mxfp4(w.to(torch.bfloat16))
    assert int(s2[0, 0]) == 127 - 30 - 2 and int(s2.max()) == 127 + 20 - 2


def test_requantisation_keeps_the_values():
    w = _rows()
    codes, scales = quantize_mxfp4(w)
    dq = dequantize_mxfp4(codes, scales, torch.bfloat16)
    c2, s2 = quantize_mxfp4(dq)
    assert torch.equal(dequantize_mxfp4(c2, s2, torch.bfloat16), dq)


def test_k_shard_invariance():
    """Blocks lie along K: a row-parallel shard quantises to the bytes of the whole's slice."""
    w = _rows()
    codes, scales = quantize_mxfp4(w)
    for a, b in ((0, 32), (64, 192), (160, 320)):
        ca, sa = quantize_mxfp4(w[:, a:b])
        assert torch.equal(ca, codes[:, a // 2:b // 2]) and torch.equal(sa, scales[:, a // 32:b // 32])
    cn, sn = quantize_mxfp4(w[8:24])                         # column-parallel: rows
    assert torch.equal(cn, codes[8:24]) and torch.equal(sn, scales[8:24])


def test_k_not_a_multiple_of_32_raises():
    from kubernetes_gpu_cluster_amd.models import build_model
    from kubernetes_gpu_cluster_amd.parallel.state import ParallelState, set_state
    set_state(ParallelState(device=torch.device("cpu")))
    cfg = PRESETS["tiny-llama"].shrink(name="tiny-llama-i528", intermediate_size=528)
    model = build_model(cfg, torch.float32, torch.device("cpu"))
    with pytest.raises(ValueError, match="mxfp4.*multiple of 32"):
        quantize_model(model, "mxfp4")


# ------------------------------------------------------------------ engine
def test_engine_generates_with_the_flag_on_cpu():
    from kubernetes_gpu_cluster_amd.engine.llm_engine import LLMEngine
    from kubernetes_gpu_cluster_amd.engine.sequence import SamplingParams
    eng = LLMEngine(EngineConfig(model="tiny-llama", random_init=True, device="cpu",
                                 dtype="float32", quantization="mxfp4", max_model_len=64,
                                 max_num_seqs=2, max_num_batched_tokens=64,
                                 num_gpu_blocks_override=16))
    model = eng.executor.runner.model
    assert model.quantization == "mxfp4"
    assert all(is_mxfp4(m.weight) for l in model.layers for m in dense_projections(l))
    s = eng.add_request([5, 9, 13], SamplingParams(temperature=0.0, max_tokens=3, ignore_eos=True))
    while eng.has_unfinished():
        eng.step()
    assert len(s.output_token_ids) == 3


@pytest.mark.parametrize("name", ["tiny-llama", "tiny-qwen2"])
def test_quantized_logits_match_hf_on_dequantized_weights(name):
    pytest.importorskip("transformers")
    from test_model_parity import _engine_logits, _hf_model, _ours
    cfg = PRESETS[name]
    sd = full_state_dict_random(cfg, seed=1, std=0.05)
    model, runner = _ours(cfg, sd)
    shapes = {(i, j): tuple(m.weight.shape) for i, l in enumerate(model.layers)
              for j, m in enumerate(dense_projections(l))}
    l0 = model.layers[0]
    tails = {tuple(l0.self_attn.o_proj.weight.shape), tuple(l0.mlp.down_proj.weight.shape)}
    quantize_model(model, "mxfp4")
    assert model.quantization == "mxfp4"
    assert model.fold_rs_weights() == 0 and not model._fusable
    assert not model.silu_weights() and not model.silu_shapes() and not model.tail_shapes()
    assert not model.fused_norm_shapes() and not model.qkv_dims()
    # the quantised tail shapes are the layer's (N, K), not the stored [N, K/2] code bytes
    assert model.quant_tail_shapes() == tails
    # the four projections of every layer hold codes [N, K/2] + scales [N, K/32]
    for i, l in enumerate(model.layers):
        for j, m in enumerate(dense_projections(l)):
            w, s = m.weight, w4_scale(m.weight)
            N, K = shapes[(i, j)]
            assert is_mxfp4(w) and w.shape == (N, K // 2) and s.shape == (N, K // 32)
            assert s.dtype == torch.uint8
    assert model.embed_tokens.weight.dtype == torch.float32
    assert model.lm_head.get_weight().dtype == torch.float32
    # HF on the dequantised weights (the merged qkv / gate_up rows split back by name)
    sd_q = dict(sd)
    d = cfg.head_dim
    nq, nkv, I = cfg.num_heads * d, cfg.num_kv_heads * d, cfg.intermediate_size
    for i, l in enumerate(model.layers):
        qkv, o, gu, dn = [dequantize_mxfp4(m.weight, w4_scale(m.weight))
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
