"""``--quantization fp8`` on the MI355X: K9q (csrc/kernels/gemm_w8.hip) and the widen path
against an fp32 oracle computed on the CPU from the same e4m3 weights and scales, graph
capture of both, and a quantised engine against HF on the dequantised weights."""
import os
import subprocess
import sys

import pytest
import torch

from kubernetes_gpu_cluster_amd.models import PRESETS, build_model, full_state_dict_random
from kubernetes_gpu_cluster_amd.ops.quant import dequantize_fp8_rows, quantize_fp8_rows, w8_scale

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DT = [torch.bfloat16, torch.float16]
TOL = dict(atol=3e-2, rtol=2e-2)       # test_skinny_gemm's: the rounding points are K9's


def _oracle(x, w8, scale):
    return x.float().cpu() @ (w8.float().cpu() * scale.cpu()[:, None]).t()


def _cfgs(gemm, M, N, K, silu=False):
    return [c for c in gemm._W8_CONFIGS if gemm.w8_ok(M, N, K, c) and (not silu or c[1] == 2)]


# ------------------------------------------------------------------ K9q
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("M,N,K", [(1, 6144, 4096), (7, 4096, 14336), (16, 512, 1024),
                                   (17, 1024, 2048), (33, 2048, 512), (64, 256, 4096)])
def test_w8_gemm(gpu, dt, M, N, K):
    from kubernetes_gpu_cluster_amd.ops import gemm
    torch.manual_seed(M + N)
    x = torch.randn(M, K, dtype=dt, device=gpu)
    w8, scale = quantize_fp8_rows(torch.randn(N, K, dtype=dt, device=gpu) * K ** -0.5)
    b = torch.randn(N, dtype=dt, device=gpu)
    exp = _oracle(x, w8, scale)
    cfgs = _cfgs(gemm, M, N, K)
    assert cfgs and gemm.w8_default_cfg(M, N, K) in cfgs
    worst = 0.0
    for cfg in cfgs:
        got = gemm.w8_gemm(x, w8, scale, None, cfg).float().cpu()
        worst = max(worst, ((got - exp).abs() / (TOL["atol"] + TOL["rtol"] * exp.abs())).max().item())
        torch.testing.assert_close(got, exp, **TOL)
        gotb = gemm.w8_gemm(x, w8, scale, b, cfg).float().cpu()
        torch.testing.assert_close(gotb, exp + b.float().cpu(), **TOL)
    print(f"K9q {dt} M={M} N={N} K={K}: {len(cfgs)} cfgs, worst error / tolerance {worst:.3f}")


def test_w8_ok_rejects_what_the_kernel_cannot_run(gpu):
    from kubernetes_gpu_cluster_amd.ops import gemm
    assert not gemm.w8_ok(1, 512, 1024 + 64, (1, 1, 4, True))     # K % (64 * nw)
    assert not gemm.w8_ok(17, 512, 1024, (1, 1, 4, True))         # M > 16 * mt
    assert not gemm.w8_ok(1, 16, 1024, (1, 2, 4, True))           # N % (16 * nt)
    assert not gemm.w8_ok(64, 512, 4096, (4, 2, 16, True))        # not built
    x = torch.randn(1, 1088, dtype=torch.bfloat16, device=gpu)
    w8, scale = quantize_fp8_rows(torch.randn(512, 1088, device=gpu) * 1088 ** -0.5)
    with pytest.raises(RuntimeError, match="w8_gemm"):
        gemm.w8_gemm(x, w8, scale, None, (1, 1, 4, True))
    # ... and the dispatcher takes the widen path there
    torch.testing.assert_close(gemm.w8_linear(x, w8).float().cpu(), _oracle(x, w8, scale), **TOL)


def test_w8_gemm_zero_row_and_row_magnitudes(gpu):
    """An all-zero weight row (scale 1), and rows of magnitude x 2^k, k = -6..6: a scale
    indexed by the wrong row is off by at least a factor of 2."""
    from kubernetes_gpu_cluster_amd.ops import gemm
    torch.manual_seed(11)
    M, N, K = 5, 13 * 32, 1024
    w = torch.randn(N, K, device=gpu) * K ** -0.5
    k = torch.arange(N, device=gpu) % 13 - 6
    w = (w * (2.0 ** k)[:, None].float()).to(torch.bfloat16)
    w[37] = 0
    w8, scale = quantize_fp8_rows(w)
    assert scale[37].item() == 1.0
    x = torch.randn(M, K, dtype=torch.bfloat16, device=gpu)
    b = torch.randn(N, dtype=torch.bfloat16, device=gpu)
    exp = _oracle(x, w8, scale)
    for cfg in _cfgs(gemm, M, N, K):
        got = gemm.w8_gemm(x, w8, scale, None, cfg).float().cpu()
        torch.testing.assert_close(got, exp, **TOL)
        assert bool((got[:, 37] == 0).all())
        gotb = gemm.w8_gemm(x, w8, scale, b, cfg).float().cpu()
        torch.testing.assert_close(gotb, exp + b.float().cpu(), **TOL)
    # the widen path sees the same rows.  Its weights are rounded to bf16, an error that
    # grows with a row's magnitude (K9q's does not: it scales the fp32 sum), so each column
    # is compared on its own row's scale, 2^-k: the tolerance then is that of unit rows
    xl = torch.randn(80, K, dtype=torch.bfloat16, device=gpu)
    unit = (2.0 ** -k).float().cpu()[None, :]
    torch.testing.assert_close(gemm.w8_widen_linear(xl, w8, scale).float().cpu() * unit,
                               _oracle(xl, w8, scale) * unit, **TOL)


def test_w8_gemm_strided_x(gpu):
    """X may be a row-strided view (e.g. a slice of a wider activation)."""
    from kubernetes_gpu_cluster_amd.ops import gemm
    torch.manual_seed(3)
    big = torch.randn(8, 3072, dtype=torch.bfloat16, device=gpu)
    x = big[:, :1024]
    w8, scale = quantize_fp8_rows(torch.randn(512, 1024, dtype=torch.bfloat16, device=gpu) * 0.03)
    got = gemm.w8_gemm(x, w8, scale, None, (1, 1, 4, True))
    torch.testing.assert_close(got.float().cpu(), _oracle(x, w8, scale), **TOL)
    torch.testing.assert_close(gemm.w8_linear(x, w8).float().cpu(), _oracle(x, w8, scale), **TOL)


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("M,N,K", [(1, 28672, 4096), (5, 1024, 2048), (16, 2048, 1024),
                                   (40, 512, 4096), (64, 1024, 512)])
def test_w8_silu_matches_fp32(gpu, dt, M, N, K):
    """K9q's SiLU form over a merged [gate; up] fp8 weight [2I, K], every configuration
    holding M, vs silu(g) * u in fp32; and linear_silu takes it for an fp8 weight."""
    from kubernetes_gpu_cluster_amd.ops import gemm
    torch.manual_seed(M + N + K)
    x = torch.randn(M, K, dtype=dt, device=gpu)
    w = torch.randn(N, K, dtype=dt, device=gpu) * K ** -0.5
    w[N // 2:] *= 4.0                        # up rows on another scale than their gate rows
    w8, scale = quantize_fp8_rows(w)
    ref = _oracle(x, w8, scale)
    exp = torch.nn.functional.silu(ref[:, : N // 2]) * ref[:, N // 2:]
    cfgs = _cfgs(gemm, M, N, K, silu=True)
    assert cfgs
    for cfg in cfgs:
        out = torch.full((M, N // 2), float("nan"), dtype=dt, device=gpu)
        gemm.w8_silu(x, w8, scale, cfg, out)
        torch.testing.assert_close(out.float().cpu(), exp, **TOL)
    before = gemm.w8_counts()["k9q_silu"]
    torch.testing.assert_close(gemm.linear_silu(x, w8).float().cpu(), exp, **TOL)
    assert gemm.w8_counts()["k9q_silu"] == before + 1


# ------------------------------------------------------------------ M > 64: widen + library GEMM
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("M,N,K", [(65, 512, 1024), (200, 2048, 512)])
def test_w8_widen_path(gpu, dt, M, N, K):
    from kubernetes_gpu_cluster_amd.ops import gemm
    torch.manual_seed(M + K)
    x = torch.randn(M, K, dtype=dt, device=gpu)
    w8, scale = quantize_fp8_rows(torch.randn(N, K, dtype=dt, device=gpu) * K ** -0.5)
    b = torch.randn(N, dtype=dt, device=gpu)
    exp = _oracle(x, w8, scale)
    wide = gemm.w8_widen(w8, scale, dt)
    assert wide.dtype == dt and wide.shape == (N, K)
    assert torch.equal(wide.cpu(), dequantize_fp8_rows(w8.cpu(), scale.cpu(), dt))   # one rounding
    before = gemm.w8_counts()["widen"]
    torch.testing.assert_close(gemm.linear(x, w8).float().cpu(), exp, **TOL)
    torch.testing.assert_close(gemm.linear(x, w8, b).float().cpu(), exp + b.float().cpu(), **TOL)
    assert gemm.w8_counts()["widen"] == before + 2


def test_w8_widen_two_weights_share_the_scratch(gpu):
    from kubernetes_gpu_cluster_amd.ops import gemm
    torch.manual_seed(5)
    dt = torch.bfloat16
    x1 = torch.randn(70, 1024, dtype=dt, device=gpu)
    x2 = torch.randn(96, 512, dtype=dt, device=gpu)
    wa, sa = quantize_fp8_rows(torch.randn(768, 1024, dtype=dt, device=gpu) * 0.03)
    wb, sb = quantize_fp8_rows(torch.randn(2048, 512, dtype=dt, device=gpu) * 0.05)
    ya = gemm.linear(x1, wa)
    yb = gemm.linear(x2, wb)
    ya2 = gemm.linear(x1, wa)
    torch.cuda.synchronize()
    torch.testing.assert_close(ya.float().cpu(), _oracle(x1, wa, sa), **TOL)
    torch.testing.assert_close(yb.float().cpu(), _oracle(x2, wb, sb), **TOL)
    assert torch.equal(ya, ya2)


# ------------------------------------------------------------------ graph capture
def test_w8_paths_replay_in_a_graph(gpu):
    from kubernetes_gpu_cluster_amd.ops import gemm
    torch.manual_seed(9)
    dt = torch.bfloat16
    w8, scale = quantize_fp8_rows(torch.randn(1024, 2048, dtype=dt, device=gpu) * 0.02)
    xs = torch.zeros(8, 2048, dtype=dt, device=gpu)
    xl = torch.zeros(96, 2048, dtype=dt, device=gpu)
    gemm.w8_reserve(gpu, w8.numel(), dt)          # static before capture
    for _ in range(2):
        gemm.linear(xs, w8)
        gemm.linear(xl, w8)
    torch.cuda.synchronize()
    gs, gl = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(gs):
        ys = gemm.linear(xs, w8)                  # K9q (default configuration)
    with torch.cuda.graph(gl):
        yl = gemm.linear(xl, w8)                  # widen + library GEMM
    for seed in (1, 2):
        g = torch.Generator(device=gpu).manual_seed(seed)
        xs.copy_(torch.randn(xs.shape, device=gpu, generator=g))
        xl.copy_(torch.randn(xl.shape, device=gpu, generator=g))
        gs.replay()
        gl.replay()
        torch.cuda.synchronize()
        torch.testing.assert_close(ys.float().cpu(), _oracle(xs, w8, scale), **TOL)
        torch.testing.assert_close(yl.float().cpu(), _oracle(xl, w8, scale), **TOL)


# ------------------------------------------------------------------ engine
@pytest.mark.parametrize("name", ["tiny-llama", "tiny-qwen2", "tiny-llama-gqa8"])
def test_gpu_quantized_logits_match_hf(gpu, name):
    """test_gpu_logits_match_hf's procedure with a quantised model, against HF on the
    dequantised weights."""
    pytest.importorskip("transformers")
    from kubernetes_gpu_cluster_amd.engine.model_runner import ModelRunner
    from kubernetes_gpu_cluster_amd.models.quant import dense_projections, quantize_model
    from kubernetes_gpu_cluster_amd.ops import gemm
    from kubernetes_gpu_cluster_amd.parallel.state import ParallelState, set_state
    from test_model_parity import _engine_logits, _hf_model
    cfg = PRESETS[name]
    sd = full_state_dict_random(cfg, seed=2, std=0.05)
    set_state(ParallelState(device=gpu))
    model = build_model(cfg, torch.bfloat16, gpu)
    model.load_weights(sd.items())
    quantize_model(model)
    sd_q = dict(sd)
    d = cfg.head_dim
    nq, nkv, I = cfg.num_heads * d, cfg.num_kv_heads * d, cfg.intermediate_size
    for i, l in enumerate(model.layers):
        qkv, o, gu, dn = [dequantize_fp8_rows(m.weight, w8_scale(m.weight)).cpu()
                          for m in dense_projections(l)]
        p = f"model.layers.{i}."
        sd_q.update({p + "self_attn.q_proj.weight": qkv[:nq],
                     p + "self_attn.k_proj.weight": qkv[nq:nq + nkv],
                     p + "self_attn.v_proj.weight": qkv[nq + nkv:],
                     p + "self_attn.o_proj.weight": o, p + "mlp.gate_proj.weight": gu[:I],
                     p + "mlp.up_proj.weight": gu[I:], p + "mlp.down_proj.weight": dn})
    hf, _ = _hf_model(cfg, sd_q)
    runner = ModelRunner(model, cfg, torch.bfloat16, gpu, block_size=16, max_model_len=256,
                         max_num_seqs=4, token_budget=128, enforce_eager=True)
    runner.init_kv_cache(48)
    g = torch.Generator().manual_seed(0)
    prompt = torch.randint(3, cfg.vocab_size, (70,), generator=g).tolist()
    extra = torch.randint(3, cfg.vocab_size, (4,), generator=g).tolist()
    with torch.no_grad():
        ref = hf(torch.tensor([prompt + extra])).logits[0].float()
    gemm.clear_plan()
    c0 = gemm.w8_counts()
    got = _engine_logits(model, runner, prompt, [33, 37], extra).float().cpu()
    c1 = gemm.w8_counts()
    assert c1["k9q"] > c0["k9q"] and c1["k9q_silu"] > c0["k9q_silu"]    # both chunks: M <= 64
    scale = ref.abs().max().item()
    pos_err = (got - ref).abs().max(-1).values
    cos = torch.nn.functional.cosine_similarity(got, ref, dim=-1)
    print(f"{name}: worst position error {pos_err.max().item():.4f} of scale {scale:.3f}, "
          f"min cos {cos.min().item():.6f}")
    ok = (pos_err < 0.03 * scale + 1e-3) & (cos > 0.999)
    assert bool(ok.all()), (pos_err.max().item(), scale, cos.min().item())


def test_quantized_engine_graph_equals_eager(gpu):
    from kubernetes_gpu_cluster_amd.engine.sequence import SamplingParams
    from kubernetes_gpu_cluster_amd.ops import gemm
    from test_engine_gpu import _run, _tiny_engine
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(100, 128000, (n,), generator=g).tolist() for n in (5, 77, 300, 1)]
    params = [SamplingParams(temperature=1.0, seed=i, max_tokens=12, ignore_eos=True)
              for i in range(len(prompts))]
    outs = {}
    try:
        for eager in (True, False):
            gemm.clear_plan()
            eng = _tiny_engine(enforce_eager=eager, quantization="fp8")
            model = eng.executor.runner.model
            assert model.quantization == "fp8"
            assert model.layers[0].mlp.down_proj.weight.dtype == torch.float8_e4m3fn
            c0 = gemm.w8_counts()
            outs[eager] = _run(eng, prompts, params)
            if eager:
                # no plan: the default K9q configuration ran on the decode steps
                c1 = gemm.w8_counts()
                assert c1["k9q"] > c0["k9q"] and c1["k9q_silu"] > c0["k9q_silu"]
            else:
                assert eng.executor.runner.stats["graph_steps"] > 0
                # the plan the decode graphs were captured with: K9q at the decode buckets
                plan = gemm.w8_plan()
                assert plan and all(M <= 16 for M, _, _ in plan)
                assert any(cfg is not None for cfg in plan.values()), plan
            del eng, model
            torch.cuda.empty_cache()
    finally:
        gemm.clear_plan()
    for a, b in zip(outs[False], outs[True]):
        assert len(a) == len(b) == 12
        assert a[:4] == b[:4], (a, b)


CHILD = r'''
import torch
from kubernetes_gpu_cluster_amd import ops
assert ops.DEBUG and ops.extension_path().endswith("_kgc_ops_debug.so")
ops.load_extension(strict=True)
assert torch.ops.kgc.debug_build()
from kubernetes_gpu_cluster_amd.engine.config import EngineConfig
from kubernetes_gpu_cluster_amd.engine.llm_engine import LLMEngine
from kubernetes_gpu_cluster_amd.engine.sequence import SamplingParams
from kubernetes_gpu_cluster_amd.models import PRESETS
from kubernetes_gpu_cluster_amd.ops import gemm
PRESETS["llama-3-8b-2l"] = PRESETS["llama-3-8b"].shrink(name="llama-3-8b-2l", num_layers=2)
eng = LLMEngine(EngineConfig(model="llama-3-8b-2l", random_init=True, max_model_len=1024,
                             max_num_seqs=16, max_num_batched_tokens=2048,
                             num_gpu_blocks_override=512, cuda_graph_max_bs=4,
                             quantization="fp8"))
g = torch.Generator().manual_seed(1)
seqs = [eng.add_request(torch.randint(100, 128000, (n,), generator=g).tolist(),
                        SamplingParams(temperature=1.0, seed=n, max_tokens=6, ignore_eos=True))
        for n in (5, 77, 300)]
while eng.has_unfinished():
    eng.step()
ops.debug_check()
assert all(len(s.output_token_ids) == 6 for s in seqs)
assert eng.executor.runner.stats["graph_steps"] > 0
c = gemm.w8_counts()
assert c["k9q"] > 0 and c["widen"] > 0, c
print("W8-DEBUG-BUILD-OK", c)
'''


def test_quantized_engine_in_the_debug_build(gpu):
    """The quantised engine (prefill through the widen path, graphed K9q decode) on the
    bounds-checking library, in a child process: one process cannot load both builds."""
    so = os.path.join(ROOT, "kubernetes_gpu_cluster_amd", "_kgc_ops_debug.so")
    if not os.path.exists(so):
        pytest.fail("debug build missing: run KGC_HIP_DEBUG=1 python csrc/build.py")
    pp = os.environ.get("PYTHONPATH", "")
    env = dict(os.environ, KGC_HIP_DEBUG="1",
               PYTHONPATH=os.pathsep.join([p for p in pp.split(os.pathsep) if p] + [ROOT]))
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "W8-DEBUG-BUILD-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
