"""K9mq on the MI355X (csrc/kernels/gemm_w8_decode.hip): the K9m pipeline over packed e4m3
weights at 64 < M <= 512, against the fp32 CPU oracle of test_quant_fp8_gpu.py (the same e4m3
values and scales), its tolerance and its input scaling; the dispatcher, graph replay and the
quantised engine at a decode bucket above 64."""
import os
import subprocess
import sys

import pytest
import torch

from kubernetes_gpu_cluster_amd.ops.quant import pack_fp8_tiles_reference, quantize_fp8_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DT = [torch.bfloat16, torch.float16]
TOL = dict(atol=3e-2, rtol=2e-2)       # test_quant_fp8_gpu.py's
PARTIAL, OUT, SILU = 0, 1, 2


def _oracle(x, w8, scale):
    return x.float().cpu() @ (w8.float().cpu() * scale.cpu()[:, None]).t()


_cases: dict = {}


def _case(gpu, dt, M, N, K, up=1.0):
    """(x, w8, scale, packed, SiLU-packed or None, oracle), made once per shape and shared."""
    key = (dt, M, N, K, up)
    if key not in _cases:
        g = torch.Generator(device=gpu).manual_seed(M * 7 + N + K)
        x = torch.randn(M, K, dtype=dt, device=gpu, generator=g)
        w = torch.randn(N, K, dtype=dt, device=gpu, generator=g) * K ** -0.5
        w[N // 2:] *= up
        w8, scale = quantize_fp8_rows(w)
        _cases[key] = (x, w8, scale, _pack(w8, False), _pack(w8, True) if N % 256 == 0 else None,
                       _oracle(x, w8, scale))
    return _cases[key]


def _pack(w8, silu):
    N, K = w8.shape
    p = torch.empty(N // 128, K // 64, 8192, dtype=w8.dtype, device=w8.device)
    torch.ops.kgc.w8_dgemm_pack(p, w8, silu)
    return p


def _ncfg():
    return int(torch.ops.kgc.w8_dgemm_num_cfgs())


def test_cfg_table(gpu):
    tiles = [tuple(torch.ops.kgc.w8_dgemm_cfg_info(c)) for c in range(_ncfg())]
    assert {(256, 128), (128, 128)} <= {t[:2] for t in tiles}
    assert {3, 4} <= {t[2] for t in tiles if t[0] == 256}
    with pytest.raises(RuntimeError, match="tile config"):
        torch.ops.kgc.w8_dgemm_cfg_info(_ncfg())


@pytest.mark.parametrize("silu", [False, True])
def test_pack_kernel_matches_the_reference(gpu, silu):
    w8, _ = quantize_fp8_rows(torch.randn(256, 192, device=gpu) * 192 ** -0.5)
    got = _pack(w8, silu).view(torch.uint8).cpu()
    assert torch.equal(got, pack_fp8_tiles_reference(w8.cpu(), silu))


# M: one row into a block / into the second block / exact blocks / a ragged last block of a
# 256-row tile; N: one tile / an odd tile count; K: one step (shorter than the ring's
# prologue) / three (no walk rotation) / 16 (rotated); S = 3 at K = 1024: uneven slices
SHAPES = [(65, 128, 64, (1,)), (129, 384, 192, (1, 2, 3)), (256, 128, 1024, (1, 2)),
          (300, 384, 1024, (1, 3)), (65, 384, 1024, (2,))]


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("M,N,K,splits", SHAPES)
def test_w8_dgemm_every_cfg(gpu, dt, M, N, K, splits):
    k = torch.ops.kgc
    x, w8, scale, wp, _, exp = _case(gpu, dt, M, N, K)
    g = torch.Generator(device=gpu).manual_seed(5)
    b = torch.randn(N, dtype=dt, device=gpu, generator=g)
    res0 = torch.randn(M, N, dtype=dt, device=gpu, generator=g)
    gamma = torch.rand(N, dtype=dt, device=gpu, generator=g) + 0.5
    rn = res0.float().cpu() + exp
    norm = rn * torch.rsqrt(rn.pow(2).mean(-1, keepdim=True) + 1e-6) * gamma.float().cpu()
    worst = 0.0
    for cfg in range(_ncfg()):
        for S in splits:
            if S == 1:
                out = torch.full((M, N), float("nan"), dtype=dt, device=gpu)
                k.w8_dgemm(out, x, wp, scale, None, cfg, OUT)
                got = out.float().cpu()
                worst = max(worst, ((got - exp).abs() / (TOL["atol"] + TOL["rtol"] * exp.abs())).max().item())
                torch.testing.assert_close(got, exp, **TOL)
                k.w8_dgemm(out, x, wp, scale, b, cfg, OUT)
                torch.testing.assert_close(out.float().cpu(), exp + b.float().cpu(), **TOL)
                continue
            ws = torch.full((S, M, N), float("nan"), dtype=torch.float32, device=gpu)
            k.w8_dgemm(ws, x, wp, scale, None, cfg, PARTIAL)
            torch.testing.assert_close(ws.sum(0).cpu(), exp, **TOL)
            red = torch.empty(M, N, dtype=dt, device=gpu)
            k.splitk_reduce(red, ws)
            torch.testing.assert_close(red.float().cpu(), exp, **TOL)
            res = res0.clone()
            k.splitk_add_rms_norm(red, ws, res, gamma, 1e-6)
            torch.testing.assert_close(res.float().cpu(), rn, **TOL)
            torch.testing.assert_close(red.float().cpu(), norm, **TOL)
    print(f"K9mq {dt} M={M} N={N} K={K}: {_ncfg()} cfgs, worst error / tolerance {worst:.3f}")


def test_w8_dgemm_rejects_what_it_cannot_run(gpu):
    k = torch.ops.kgc
    dt = torch.bfloat16
    x, w8, scale, wp, _, _ = _case(gpu, dt, 65, 128, 64)
    out = torch.empty(65, 128, dtype=dt, device=gpu)
    with pytest.raises(RuntimeError, match="tile config"):
        k.w8_dgemm(out, x, wp, scale, None, _ncfg(), OUT)
    with pytest.raises(RuntimeError, match="64 < M"):
        k.w8_dgemm(out[:64], x[:64], wp, scale, None, 0, OUT)
    with pytest.raises(RuntimeError, match="K / 64"):
        k.w8_dgemm(torch.empty(2, 65, 128, device=gpu), x, wp, scale, None, 0, PARTIAL)
    with pytest.raises(RuntimeError, match="scale"):
        k.w8_dgemm(out, x, wp, scale[:64], None, 0, OUT)
    with pytest.raises(RuntimeError, match="X"):
        k.w8_dgemm(out, x.to(torch.float16), wp, scale, None, 0, OUT)


@pytest.mark.parametrize("dt", DT)
def test_guard_rows_stay_untouched(gpu, dt):
    """out is the first M rows of a NaN-filled [M + 3, N] buffer: rows >= M are never stored."""
    k = torch.ops.kgc
    M, N, K = 129, 256, 192
    x, w8, scale, wp, wps, _ = _case(gpu, dt, M, N, K)
    for cfg in range(_ncfg()):
        buf = torch.full((M + 3, N), float("nan"), dtype=dt, device=gpu)
        k.w8_dgemm(buf[:M], x, wp, scale, None, cfg, OUT)
        assert bool(torch.isfinite(buf[:M]).all()) and bool(torch.isnan(buf[M:]).all())
        buf = torch.full((M + 3, N // 2), float("nan"), dtype=dt, device=gpu)
        k.w8_dgemm(buf[:M], x, wps, scale, None, cfg, SILU)
        assert bool(torch.isfinite(buf[:M]).all()) and bool(torch.isnan(buf[M:]).all())


def test_zero_row_and_row_magnitudes(gpu):
    """test_w8_gemm_zero_row_and_row_magnitudes's weight: rows x 2^k, k = n % 13 - 6, and one
    all-zero row -- a scale indexed by the wrong row is off by at least a factor of 2."""
    k = torch.ops.kgc
    torch.manual_seed(11)
    M, N, K = 80, 384, 1024
    w = torch.randn(N, K, device=gpu) * K ** -0.5
    e = torch.arange(N, device=gpu) % 13 - 6
    w = (w * (2.0 ** e)[:, None].float()).to(torch.bfloat16)
    w[37] = 0
    w8, scale = quantize_fp8_rows(w)
    assert scale[37].item() == 1.0
    x = torch.randn(M, K, dtype=torch.bfloat16, device=gpu)
    exp = _oracle(x, w8, scale)
    wp = _pack(w8, False)
    for cfg in range(_ncfg()):
        out = torch.empty(M, N, dtype=x.dtype, device=gpu)
        k.w8_dgemm(out, x, wp, scale, None, cfg, OUT)
        torch.testing.assert_close(out.float().cpu(), exp, **TOL)
        assert bool((out[:, 37] == 0).all())
        ws = torch.empty(2, M, N, dtype=torch.float32, device=gpu)
        k.w8_dgemm(ws, x, wp, scale, None, cfg, PARTIAL)
        torch.testing.assert_close(ws.sum(0).cpu(), exp, **TOL)
        assert bool((ws[:, :, 37] == 0).all())


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("M,I", [(65, 128), (200, 256), (200, 128), (65, 256)])
def test_silu_form(gpu, dt, M, I):
    """The SiLU epilogue and the S = 2 slices + splitk_reduce_silu over a merged [gate; up]
    weight whose up rows sit on another scale; linear_silu takes an installed entry."""
    from kubernetes_gpu_cluster_amd.ops import gemm
    k = torch.ops.kgc
    N, K = 2 * I, 1024
    x, w8, scale, _, _, ref = _case(gpu, dt, M, N, K, up=4.0)
    exp = torch.nn.functional.silu(ref[:, :I]) * ref[:, I:]
    assert gemm.pack_w8_decode_weights([], [w8]) in (0, N * K)
    for cfg in range(_ncfg()):
        got = gemm.w8_dgemm(x, w8, cfg, 1, epi=SILU)
        torch.testing.assert_close(got.float().cpu(), exp, **TOL)
        red = torch.empty(M, I, dtype=dt, device=gpu)
        k.splitk_reduce_silu(red, gemm.w8_dgemm(x, w8, cfg, 2, silu_w=True), True)
        torch.testing.assert_close(red.float().cpu(), exp, **TOL)
    try:
        for plan in ((0, 1), (_ncfg() - 1, 2)):
            gemm._plan_w8_dg[(M, N, K, "silu")] = plan
            before = gemm.w8_counts()["k9mq_silu"]
            torch.testing.assert_close(gemm.linear_silu(x, w8).float().cpu(), exp, **TOL)
            assert gemm.w8_counts()["k9mq_silu"] == before + 1
    finally:
        gemm.clear_plan()


def test_strided_x(gpu):
    """X may be a row-strided view: a [96, 1024] slice of a [96, 3072] buffer."""
    from kubernetes_gpu_cluster_amd.ops import gemm
    torch.manual_seed(3)
    big = torch.randn(96, 3072, dtype=torch.bfloat16, device=gpu)
    x = big[:, 1024:2048]
    w8, scale = quantize_fp8_rows(torch.randn(512, 1024, dtype=torch.bfloat16, device=gpu) * 0.03)
    exp = _oracle(x, w8, scale)
    gemm.pack_w8_decode_weights([w8], [])
    for cfg in range(_ncfg()):
        torch.testing.assert_close(gemm.w8_dgemm(x, w8, cfg, 1).float().cpu(), exp, **TOL)
        ws = gemm.w8_dgemm(x, w8, cfg, 2)
        torch.testing.assert_close(ws.sum(0).cpu(), exp, **TOL)


def test_dispatcher_takes_the_plan_and_falls_back(gpu):
    from kubernetes_gpu_cluster_amd.ops import gemm
    torch.manual_seed(4)
    dt = torch.bfloat16
    M, N, K = 96, 512, 1024
    x = torch.randn(M, K, dtype=dt, device=gpu)
    w8, scale = quantize_fp8_rows(torch.randn(N, K, dtype=dt, device=gpu) * K ** -0.5)
    b = torch.randn(N, dtype=dt, device=gpu)
    exp = _oracle(x, w8, scale)
    gemm.clear_plan()
    try:
        # an entry, but no packed copy: the widen path
        gemm._plan_w8_dg[(M, N, K, "plain")] = (2, 1)
        c0 = gemm.w8_counts()
        torch.testing.assert_close(gemm.linear(x, w8).float().cpu(), exp, **TOL)
        c1 = gemm.w8_counts()
        assert c1["widen"] == c0["widen"] + 1 and c1["k9mq"] == c0["k9mq"]
        assert gemm.pack_w8_decode_weights([w8], []) == N * K
        assert gemm.pack_w8_decode_weights([w8], []) == 0            # packed once
        torch.testing.assert_close(gemm.linear(x, w8).float().cpu(), exp, **TOL)
        torch.testing.assert_close(gemm.linear(x, w8, b).float().cpu(), exp + b.float().cpu(), **TOL)
        c2 = gemm.w8_counts()
        assert c2["k9mq"] == c1["k9mq"] + 2 and c2["widen"] == c1["widen"]
        # split-K: slices + splitk_reduce; with a bias, the widen path
        gemm._plan_w8_dg[(M, N, K, "plain")] = (3, 4)
        torch.testing.assert_close(gemm.linear(x, w8).float().cpu(), exp, **TOL)
        torch.testing.assert_close(gemm.linear(x, w8, b).float().cpu(), exp + b.float().cpu(), **TOL)
        c3 = gemm.w8_counts()
        assert c3["k9mq"] == c2["k9mq"] + 1 and c3["widen"] == c2["widen"] + 1
        # a None entry, another M, the knob off: the widen path
        gemm._plan_w8_dg[(M, N, K, "plain")] = None
        gemm.linear(x, w8)
        gemm._plan_w8_dg[(M, N, K, "plain")] = (2, 1)
        gemm.linear(x[:80], w8)
        mode, gemm.W8.dgemm_mode = gemm.W8.dgemm_mode, "0"
        try:
            gemm.linear(x, w8)
        finally:
            gemm.W8.dgemm_mode = mode
        c4 = gemm.w8_counts()
        assert c4["k9mq"] == c3["k9mq"] and c4["widen"] == c3["widen"] + 3
        gemm.clear_plan()
        torch.testing.assert_close(gemm.linear(x, w8).float().cpu(), exp, **TOL)
        c5 = gemm.w8_counts()
        assert c5["k9mq"] == c4["k9mq"] and c5["widen"] == c4["widen"] + 1
    finally:
        gemm.clear_plan()


def test_paths_replay_in_a_graph(gpu):
    """linear, linear_silu and linear_add_rms at M = 96 with entries installed, captured and
    replayed on two fresh inputs."""
    from kubernetes_gpu_cluster_amd.ops import gemm
    torch.manual_seed(9)
    dt = torch.bfloat16
    M, K, N, I = 96, 1024, 512, 256
    w8, scale = quantize_fp8_rows(torch.randn(N, K, dtype=dt, device=gpu) * K ** -0.5)
    wo, so = quantize_fp8_rows(torch.randn(N, K, dtype=dt, device=gpu) * K ** -0.5)
    wg = torch.randn(2 * I, K, dtype=dt, device=gpu) * K ** -0.5
    wg[I:] *= 4.0
    wg8, sg = quantize_fp8_rows(wg)
    gamma = torch.rand(N, dtype=dt, device=gpu) + 0.5
    x = torch.zeros(M, K, dtype=dt, device=gpu)
    res = torch.zeros(M, N, dtype=dt, device=gpu)
    gemm.clear_plan()
    gemm.pack_w8_decode_weights([w8, wo], [wg8])
    try:
        gemm._plan_w8_dg[(M, N, K, "plain")] = (2, 2)
        gemm._plan_w8_dg[(M, 2 * I, K, "silu")] = (3, 1)
        gemm._plan_w8_dg[(M, N, K, "tail")] = (4, 2)

        def body():
            return (gemm.linear(x, w8), gemm.linear_silu(x, wg8),
                    gemm.linear_add_rms(x, wo, res, gamma, 1e-6)[0])
        c0 = gemm.w8_counts()
        body()
        c1 = gemm.w8_counts()
        assert (c1["k9mq"], c1["k9mq_silu"], c1["widen"]) == (c0["k9mq"] + 2, c0["k9mq_silu"] + 1,
                                                              c0["widen"])
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            y, a, nrm = body()
        for seed in (1, 2):
            gen = torch.Generator(device=gpu).manual_seed(seed)
            x.copy_(torch.randn(x.shape, device=gpu, generator=gen))
            r0 = torch.randn(res.shape, device=gpu, generator=gen).to(dt)
            res.copy_(r0)
            g.replay()
            torch.cuda.synchronize()
            torch.testing.assert_close(y.float().cpu(), _oracle(x, w8, scale), **TOL)
            gu = _oracle(x, wg8, sg)
            torch.testing.assert_close(a.float().cpu(),
                                       torch.nn.functional.silu(gu[:, :I]) * gu[:, I:], **TOL)
            rn = r0.float().cpu() + _oracle(x, wo, so)
            torch.testing.assert_close(res.float().cpu(), rn, **TOL)
            exp = rn * torch.rsqrt(rn.pow(2).mean(-1, keepdim=True) + 1e-6) * gamma.float().cpu()
            torch.testing.assert_close(nrm.float().cpu(), exp, **TOL)
    finally:
        gemm.clear_plan()


# ------------------------------------------------------------------ engine
def test_quantized_engine_at_a_mid_bucket(gpu):
    """80 sequences decode in the 80-row bucket: K9mq in force mode, graph against eager (both
    run identical kernels), and the knob at 0 (the widen path, no packed copies)."""
    from kubernetes_gpu_cluster_amd.engine.sequence import SamplingParams
    from kubernetes_gpu_cluster_amd.ops import gemm
    from test_engine_gpu import _run, _tiny_engine
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(100, 128000, (int(n),), generator=g).tolist()
               for n in torch.randint(1, 12, (80,), generator=g)]
    params = [SamplingParams(temperature=1.0, seed=i, max_tokens=6, ignore_eos=True)
              for i in range(len(prompts))]
    outs = {}
    mode = gemm.W8.dgemm_mode
    try:
        for name, knob, eager in (("graph", "force", False), ("eager", "force", True),
                                  ("off", "0", False)):
            gemm.clear_plan()
            gemm.W8.dgemm_mode = knob
            c0 = gemm.w8_counts()      # (a graph engine's GEMM calls are counted at capture)
            eng = _tiny_engine(enforce_eager=eager, quantization="fp8", max_num_seqs=96,
                               cuda_graph_max_bs=128)
            outs[name] = _run(eng, prompts, params)
            c1 = gemm.w8_counts()
            if knob == "0":
                assert c1["k9mq"] == c0["k9mq"] and c1["k9mq_silu"] == c0["k9mq_silu"]
                assert not gemm.w8_dg_plan()
            else:
                assert any(k[0] > 64 and v is not None for k, v in gemm.w8_dg_plan().items())
                assert c1["k9mq"] > c0["k9mq"] and c1["k9mq_silu"] > c0["k9mq_silu"]
            if not eager:
                assert eng.executor.runner.stats["graph_steps"] > 0
            del eng
            torch.cuda.empty_cache()
    finally:
        gemm.W8.dgemm_mode = mode
        gemm.clear_plan()
    assert all(len(o) == 6 for v in outs.values() for o in v)
    for a, b in zip(outs["graph"], outs["eager"]):
        assert a[:4] == b[:4], (a, b)
    same = sum(a[0] == b[0] for a, b in zip(outs["graph"], outs["off"]))
    print(f"first tokens, K9mq (force) vs the widen path: {same} / {len(prompts)} agree")


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
assert gemm.W8.dgemm_mode == "force"
PRESETS["llama-3-8b-2l"] = PRESETS["llama-3-8b"].shrink(name="llama-3-8b-2l", num_layers=2)
eng = LLMEngine(EngineConfig(model="llama-3-8b-2l", random_init=True, max_model_len=1024,
                             max_num_seqs=96, max_num_batched_tokens=2048,
                             num_gpu_blocks_override=512, cuda_graph_max_bs=80,
                             quantization="fp8"))
g = torch.Generator().manual_seed(1)
seqs = [eng.add_request(torch.randint(100, 128000, (1 + n % 7,), generator=g).tolist(),
                        SamplingParams(temperature=1.0, seed=n, max_tokens=4, ignore_eos=True))
        for n in range(80)]
while eng.has_unfinished():
    eng.step()
ops.debug_check()
assert all(len(s.output_token_ids) == 4 for s in seqs)
assert eng.executor.runner.stats["graph_steps"] > 0
c = gemm.w8_counts()
assert c["k9mq"] > 0 and c["k9mq_silu"] > 0, c
assert any(k[0] > 64 for k in gemm.w8_dg_plan())
print("W8-MID-DEBUG-BUILD-OK", c)
'''


def test_quantized_mid_bucket_engine_in_the_debug_build(gpu):
    """The quantised engine with a decode bucket above 64 (K9mq, force mode) on the
    bounds-checking library, in a child process: one process cannot load both builds."""
    so = os.path.join(ROOT, "kubernetes_gpu_cluster_amd", "_kgc_ops_debug.so")
    if not os.path.exists(so):
        pytest.fail("debug build missing: run KGC_HIP_DEBUG=1 python csrc/build.py")
    pp = os.environ.get("PYTHONPATH", "")
    env = dict(os.environ, KGC_HIP_DEBUG="1", KGC_W8_DGEMM="force",
               PYTHONPATH=os.pathsep.join([p for p in pp.split(os.pathsep) if p] + [ROOT]))
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "W8-MID-DEBUG-BUILD-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
