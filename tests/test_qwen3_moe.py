"""Qwen3-MoE (128 experts, top-8, Qwen3 attention) on the CPU: config parsing, presets,
checkpoint names and float32 parity with transformers."""
import pytest
import torch

from kubernetes_gpu_cluster_amd.models import PRESETS, build_model, full_state_dict_random
from kubernetes_gpu_cluster_amd.models.configs import config_from_hf, resolve_model
from kubernetes_gpu_cluster_amd.parallel.state import ParallelState, set_state

from test_model_parity import _engine_logits, _ours

HF_CFG = {"model_type": "qwen3_moe", "hidden_size": 2048, "num_hidden_layers": 48,
          "num_attention_heads": 32, "num_key_value_heads": 4, "head_dim": 128,
          "intermediate_size": 6144, "moe_intermediate_size": 768, "num_experts": 128,
          "num_experts_per_tok": 8, "norm_topk_prob": True, "vocab_size": 151936,
          "max_position_embeddings": 40960, "rope_theta": 1000000.0, "rms_norm_eps": 1e-6,
          "decoder_sparse_step": 1, "mlp_only_layers": [], "bos_token_id": 151643,
          "eos_token_id": 151645}


def test_config_from_hf_and_presets():
    cfg = config_from_hf(HF_CFG, "Qwen3-30B-A3B")
    assert (cfg.arch, cfg.qk_norm, cfg.num_experts, cfg.top_k_experts) == ("qwen3", True, 128, 8)
    assert (cfg.intermediate_size, cfg.head_dim, cfg.norm_topk_prob) == (768, 128, True)
    assert config_from_hf({**HF_CFG, "norm_topk_prob": False}, "x").norm_topk_prob is False
    preset = resolve_model("Qwen/Qwen3-30B-A3B")[0]
    assert preset is PRESETS["qwen3-30b-a3b"]
    assert cfg.shrink(name=preset.name) == preset
    tiny = resolve_model("tiny-qwen3-moe")[0]
    assert (tiny.num_experts, tiny.top_k_experts, tiny.hidden_size, tiny.intermediate_size,
            tiny.qk_norm) == (128, 8, 256, 128, True)


@pytest.mark.parametrize("field,value", [("mlp_only_layers", [0, 3]), ("decoder_sparse_step", 2)])
def test_mixed_dense_sparse_stack_refused(field, value):
    with pytest.raises(ValueError, match=field):
        config_from_hf({**HF_CFG, field: value}, "x")


def test_logits_match_hf():
    transformers = pytest.importorskip("transformers")
    cfg = PRESETS["tiny-qwen3-moe"]
    sd = full_state_dict_random(cfg, seed=1, std=0.05)
    hf = transformers.Qwen3MoeForCausalLM(transformers.Qwen3MoeConfig(
        vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_layers,
        num_attention_heads=cfg.num_heads, num_key_value_heads=cfg.num_kv_heads,
        head_dim=cfg.head_dim, intermediate_size=cfg.intermediate_size,
        moe_intermediate_size=cfg.intermediate_size, num_experts=cfg.num_experts,
        num_experts_per_tok=cfg.top_k_experts, norm_topk_prob=cfg.norm_topk_prob,
        decoder_sparse_step=1, mlp_only_layers=[], rms_norm_eps=cfg.rms_eps,
        max_position_embeddings=cfg.max_position, tie_word_embeddings=False,
        rope_parameters={"rope_theta": cfg.rope_theta, "rope_type": "default"})).eval()
    hsd = {k: v for k, v in sd.items() if ".experts." not in k}
    for i in range(cfg.num_layers):
        p = f"model.layers.{i}.mlp.experts."
        w = {n: torch.stack([sd[p + f"{e}.{n}.weight"] for e in range(cfg.num_experts)])
             for n in ("gate_proj", "up_proj", "down_proj")}
        hsd[p + "gate_up_proj"] = torch.cat([w["gate_proj"], w["up_proj"]], 1)
        hsd[p + "down_proj"] = w["down_proj"]
    missing, unexpected = hf.load_state_dict(hsd, strict=False)
    assert not unexpected and all("rotary" in k for k in missing), (missing, unexpected)
    model, runner = _ours(cfg, sd)
    prompt = torch.randint(3, cfg.vocab_size, (40,), generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        ref = hf(prompt[None]).logits[0].float()
    got = _engine_logits(model, runner, prompt.tolist(), [16, 24], [])
    torch.testing.assert_close(got, ref, atol=2e-4, rtol=2e-4)
    # the fused transformers-v5 names load the same tensors as the per-expert hub names
    set_state(ParallelState())
    fused = build_model(cfg, torch.float32, torch.device("cpu"))
    assert fused.load_weights(hsd.items()) > 0
    for (n, a), b in zip(model.state_dict().items(), fused.state_dict().values()):
        assert torch.equal(a, b), n


def test_quantised_qwen3_moe_refused_at_startup():
    from kubernetes_gpu_cluster_amd.engine.config import EngineConfig
    from kubernetes_gpu_cluster_amd.engine.llm_engine import LLMEngine
    with pytest.raises(ValueError, match="MoE model 'tiny-qwen3-moe'"):
        LLMEngine(EngineConfig(model="tiny-qwen3-moe", random_init=True, device="cpu",
                               quantization="fp8", max_model_len=64, max_num_seqs=2,
                               max_num_batched_tokens=64, num_gpu_blocks_override=16))
