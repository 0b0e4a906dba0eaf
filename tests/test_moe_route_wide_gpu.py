"""K13w on the MI355X: the wide router kernels (64 < E <= 256 experts, top-k <= 16) against
high-precision references, the grouped expert MLP at 128 experts, and the tiny-qwen3-moe
engine (decode graphs == eager, logits against the CPU float32 engine)."""
import pytest
import torch

from kubernetes_gpu_cluster_amd import ops
from kubernetes_gpu_cluster_amd.ops import reference as ref

from test_kernels_gpu import _tol

pytestmark = pytest.mark.gpu
DT = [torch.bfloat16, torch.float16]
GATE_SHAPES = [(128, 8, 2048), (96, 4, 256), (256, 8, 1024), (65, 2, 512)]


@pytest.mark.parametrize("renorm", [True, False])
@pytest.mark.parametrize("dt", DT + [torch.float32])
@pytest.mark.parametrize("E,k", [(65, 1), (96, 4), (128, 8), (256, 8), (200, 16)])
def test_route_wide(gpu, dt, E, k, renorm):
    torch.manual_seed(5)
    logits = torch.randn(300, E + 3, dtype=dt, device=gpu)[:, :E]      # non-contiguous rows
    w, ids = ops.moe_topk_softmax(logits, k, renorm)
    lc = logits.cpu().float()
    rw, rids = ref.moe_topk_softmax(lc, k, renorm)
    ids, rids = ids.cpu().long(), rids.long()
    # low-precision logits tie; the kernel breaks ties by lowest id, torch.topk arbitrarily
    torch.testing.assert_close(lc.gather(1, ids), lc.gather(1, rids), atol=0, rtol=0)
    untied = (lc.gather(1, rids)[:, :, None] == lc[:, None, :]).sum(-1).eq(1).all(1)
    assert untied.any() and torch.equal(ids[untied], rids[untied])
    torch.testing.assert_close(w.cpu(), rw, atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("E,k", [(65, 1), (128, 8), (200, 16)])
def test_route_wide_all_equal_row_takes_lowest_ids(gpu, dt, E, k):
    """Contiguous rows (the vector loads): a row of equal logits returns ids 0..k-1, the
    rows around it the reference's choice."""
    torch.manual_seed(E)
    logits = torch.randn(9, E, device=gpu).to(dt)
    logits[3] = 0.25
    w, ids = ops.moe_topk_softmax(logits, k)
    assert ids[3].tolist() == list(range(k))
    lc = logits.cpu().float()
    rw, rids = ref.moe_topk_softmax(lc, k)
    torch.testing.assert_close(lc.gather(1, ids.cpu().long()), lc.gather(1, rids.long()),
                               atol=0, rtol=0)
    torch.testing.assert_close(w.cpu(), rw, atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("E,k,H", GATE_SHAPES)
@pytest.mark.parametrize("T", [1, 17, 300])
def test_gate_route_wide_exact(gpu, dt, E, k, H, T):
    """One-hot activations sweeping every column of H (every wave's K slice, every k-chunk)
    against gate columns that are permutations of (e - E/2) / 16: exact in bf16 / f16,
    untied, so ids and their order must equal the reference on every row."""
    g = torch.Generator().manual_seed(E + T)
    # an odd stride: distinct columns, every position inside the 8-element fragments
    hot = (int(torch.randint(0, H, (1,), generator=g)) + torch.arange(T) * ((H // T) | 1)) % H
    x = torch.zeros(T, H)
    x[torch.arange(T), hot] = 1.0
    wg = torch.stack([torch.randperm(E, generator=g) for _ in range(H)], 1).float()
    wg = (wg - E // 2) / 16
    got = ops.moe_gate_topk(x.to(dt).to(gpu), wg.to(dt).to(gpu), k)
    assert got is not None
    rw, rids = ref.moe_topk_softmax(x @ wg.t(), k)
    assert torch.equal(got[1].cpu(), rids)
    torch.testing.assert_close(got[0].cpu(), rw, atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("E,k,H", GATE_SHAPES + [(48, 4, 512)])
@pytest.mark.parametrize("T", [1, 17, 256, 1000])
def test_gate_route_wide_dense(gpu, dt, E, k, H, T):
    """Dense random inputs against a float64 GEMM rounded to the dtype.  No row is left out:
    the reference logits at the kernel's ids match the reference top-k values, and the
    weights are the softmax of the reference logits evaluated at the kernel's own ids."""
    torch.manual_seed(E * 100 + T + H)
    x = (torch.randn(T, H, device=gpu) * 0.5).to(dt)
    wg = (torch.randn(E, H, device=gpu) / H ** 0.5).to(dt)
    renorm = E != 96
    got = ops.moe_gate_topk(x, wg, k, renorm)
    assert got is not None
    w, ids = got[0].cpu(), got[1].cpu().long()
    logits = (x.double().cpu() @ wg.double().cpu().t()).to(dt).float()
    assert all(len(set(r)) == k for r in ids.tolist())
    sel = logits.gather(1, ids)
    torch.testing.assert_close(sel.sort(1, descending=True).values, logits.topk(k, 1).values,
                               atol=2e-2, rtol=2e-2)
    p = torch.softmax(logits, -1).gather(1, ids)
    torch.testing.assert_close(w, p / p.sum(-1, keepdim=True) if renorm else p,
                               atol=2e-2, rtol=2e-2)


def test_gate_route_wide_declines_other_shapes(gpu):
    x = torch.zeros(4, 384, dtype=torch.bfloat16, device=gpu)
    assert ops.moe_gate_topk(x, torch.zeros(128, 384, dtype=torch.bfloat16, device=gpu), 8) is None
    assert ops.moe_gate_topk(x[:, :256], torch.zeros(300, 256, dtype=torch.bfloat16, device=gpu),
                             8) is None


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("T", [1, 64, 300])
def test_fused_moe_128_experts(gpu, dt, T):
    """Many empty buckets, and buckets of under one row per expert on average."""
    E, k, H, I = 128, 8, 256, 128
    g = torch.Generator().manual_seed(T)
    x = (torch.randn(T, H, generator=g) * 0.5).to(dt)
    w13 = (torch.randn(E, 2 * I, H, generator=g) / H ** 0.5).to(dt)
    w2 = (torch.randn(E, H, I, generator=g) / I ** 0.5).to(dt)
    tw, tid = ref.moe_topk_softmax(torch.randn(T, E, generator=g), k)
    out = ops.fused_moe(x.to(gpu), w13.to(gpu), w2.to(gpu), tw.to(gpu), tid.to(gpu))
    exp = ref.moe_mlp_local(x, w13, w2, tw, tid)
    torch.testing.assert_close(out.cpu().float(), exp.float(), **_tol(dt))


def _tiny_qwen3_moe_sd(seed):
    """tiny-qwen3-moe's random state dict with the router at half the default scale."""
    from kubernetes_gpu_cluster_amd.models import PRESETS, full_state_dict_random
    cfg = PRESETS["tiny-qwen3-moe"]
    sd = full_state_dict_random(cfg, seed=seed, std=0.05)
    return cfg, {n: w * 0.5 if n.endswith("mlp.gate.weight") else w for n, w in sd.items()}


def test_tiny_qwen3_moe_graphs_equal_eager(gpu, tmp_path):
    import json
    from safetensors.torch import save_file
    from kubernetes_gpu_cluster_amd.engine.llm_engine import LLM
    from kubernetes_gpu_cluster_amd.engine.sequence import SamplingParams
    cfg, sd = _tiny_qwen3_moe_sd(5)
    save_file({n: w.contiguous() for n, w in sd.items()}, str(tmp_path / "model.safetensors"))
    json.dump({"model_type": "qwen3_moe", "hidden_size": cfg.hidden_size,
               "num_hidden_layers": cfg.num_layers, "num_attention_heads": cfg.num_heads,
               "num_key_value_heads": cfg.num_kv_heads, "head_dim": cfg.head_dim,
               "intermediate_size": 512, "moe_intermediate_size": cfg.intermediate_size,
               "num_experts": cfg.num_experts, "num_experts_per_tok": cfg.top_k_experts,
               "norm_topk_prob": True, "vocab_size": cfg.vocab_size,
               "max_position_embeddings": 512, "rope_theta": cfg.rope_theta,
               "rms_norm_eps": cfg.rms_eps, "eos_token_id": 2, "bos_token_id": 1},
              open(tmp_path / "config.json", "w"))
    prompts = [list(range(3, 40)), [5, 6, 7] * 20, [9, 10, 11]]
    sp = [SamplingParams(temperature=0, max_tokens=8, ignore_eos=True)] * 3
    outs = []
    for eager in (False, True):
        llm = LLM(str(tmp_path), device="cuda", dtype="bfloat16", max_model_len=256,
                  max_num_seqs=4, enforce_eager=eager, max_num_batched_tokens=128,
                  num_gpu_blocks_override=64)
        outs.append([o.output_token_ids for o in llm.generate(prompts, sp)])
        assert eager or llm.engine.executor.runner.stats["graph_steps"] > 0
        llm.shutdown()
    assert outs[0] == outs[1], outs


def test_tiny_qwen3_moe_logits_match_cpu_float32(gpu):
    """Prefill + decode logits through the HIP kernels (bf16) against the CPU float32 engine,
    by test_gpu_logits_match_hf's criterion and its MoE share of 0.93.  The reference pair
    alone (CPU engine in bf16 against the CPU engine in float32, this seed and prompt)
    clears it at 0.986 with the router at half the default random scale; at the default
    scale it gave 0.878, and wider routers less (x2 0.797, x4 0.743: bf16 logits of a larger
    magnitude move the softmax weights themselves), so the router is narrowed, not widened."""
    from kubernetes_gpu_cluster_amd.engine.model_runner import ModelRunner
    from kubernetes_gpu_cluster_amd.models import build_model
    from kubernetes_gpu_cluster_amd.parallel.state import ParallelState, set_state
    from test_model_parity import _engine_logits, _ours
    cfg, sd = _tiny_qwen3_moe_sd(2)
    g = torch.Generator().manual_seed(0)
    prompt = torch.randint(3, cfg.vocab_size, (70,), generator=g).tolist()
    extra = torch.randint(3, cfg.vocab_size, (4,), generator=g).tolist()
    exp = _engine_logits(*_ours(cfg, sd), prompt, [33, 37], extra).float()
    set_state(ParallelState(device=gpu))
    model = build_model(cfg, torch.bfloat16, gpu)
    model.load_weights(sd.items())
    runner = ModelRunner(model, cfg, torch.bfloat16, gpu, block_size=16, max_model_len=256,
                         max_num_seqs=4, token_budget=128, enforce_eager=True)
    runner.init_kv_cache(48)
    got = _engine_logits(model, runner, prompt, [33, 37], extra).float().cpu()
    scale = exp.abs().max().item()
    pos_err = (got - exp).abs().max(-1).values
    cos = torch.nn.functional.cosine_similarity(got, exp, dim=-1)
    ok = (pos_err < 0.03 * scale + 1e-3) & (cos > 0.999)
    assert ok.float().mean() >= 0.93, (pos_err.max(), ok.float().mean())
