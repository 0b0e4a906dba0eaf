"""``--quantization mxfp4`` on the MI355X: K9f and ``w4_widen`` (csrc/kernels/gemm_w4.hip)
against the plain-torch dequantiser and an fp32 oracle computed on the CPU from the same codes
and scales, the dispatcher, graph capture, and a quantised engine, graph against eager."""
import os
import subprocess
import sys

import pytest
import torch

from kubernetes_gpu_cluster_amd.ops.quant import (attach_w4_scale, dequantize_mxfp4,
                                                  mxfp4_exp_range, quantize_fp8_rows,
                                                  quantize_mxfp4)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DT = [torch.bfloat16, torch.float16]
TOL = dict(atol=3e-2, rtol=2e-2)       # test_skinny_gemm's: the only rounding is the output's


def _weight(N, K, dt, gpu, seed=0, spread=9):
    """An mxfp4 weight that exposes a misassigned scale or k-permutation: block kb of row n
    is on the scale 2^((kb + 3 n) % 19 - 9) (f16: the spread its exponent range holds), so
    neighbouring blocks and neighbouring rows differ; block 1 of row 2 is zero."""
    g = torch.Generator().manual_seed(seed)
    if dt == torch.float16:
        spread = 4
    e = (torch.arange(K // 32)[None, :] + 3 * torch.arange(N)[:, None]) % (2 * spread + 1) - spread
    w = torch.randn(N, K, generator=g) * K ** -0.5
    w = (w.view(N, K // 32, 32) * (2.0 ** e)[:, :, None].float()).view(N, K)
    w[2 % N, 32:64] = 0
    codes, scales = quantize_mxfp4(w.to(dt))
    assert scales[1].unique().numel() >= 3 and not torch.equal(scales[0], scales[1])
    return attach_w4_scale(codes.to(gpu), scales.to(gpu)), scales.to(gpu), \
        dequantize_mxfp4(codes, scales)                      # fp32 on the CPU: the oracle's


def _x(M, K, dt, gpu, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) * (0.25 + (torch.arange(K) % 7).float() / 4)[None, :]
    return x.to(dt).to(gpu)


def _oracle(x, dq):
    return x.float().cpu() @ dq.t()


# ------------------------------------------------------------------ w4_widen
@pytest.mark.parametrize("dt", DT)
def test_w4_widen_is_exact_for_every_byte_and_exponent(gpu, dt):
    """A [16, 512] weight whose bytes enumerate all 256 values; its 16 x 16 blocks carry
    distinct in-range exponents (both extremes, 127, neighbours differing by one).  This
    fixes the nibble order and the scale indexing of the conversion."""
    from kubernetes_gpu_cluster_amd.ops import gemm
    lo, hi = mxfp4_exp_range(dt)
    codes = torch.arange(16 * 256, dtype=torch.int32).remainder(256).to(torch.uint8).view(16, 256)
    codes = torch.roll(codes, 5, 1)                 # bytes not aligned with the blocks
    assert len(set(codes.flatten().tolist())) == 256
    span = hi - lo + 1
    b = (torch.arange(256) * 37) % span + lo + 127  # 37 is coprime to both spans
    b[0], b[1], b[2], b[3], b[4] = lo + 127, hi + 127, 127, 126, 128
    b[255], b[254] = hi + 127, hi + 126
    scales = b.to(torch.uint8).view(16, 16).contiguous()
    assert int(scales.min()) == lo + 127 and int(scales.max()) == hi + 127
    exp = dequantize_mxfp4(codes, scales, dt)
    assert torch.isfinite(exp).all()
    got = gemm.w4_widen(codes.to(gpu), scales.to(gpu), dt)
    assert got.dtype == dt and got.shape == (16, 512)
    assert torch.equal(got.cpu(), exp)
    # the dequantiser on the GPU's own torch agrees too
    assert torch.equal(dequantize_mxfp4(codes.to(gpu), scales.to(gpu), dt).cpu(), exp)


# ------------------------------------------------------------------ K9f
def _cfg_id(c):
    return "mt%d-nt%d-nw%d" % c


CFGS = [(mt, nt, nw) for mt in (1, 2, 4) for nt in (1, 2) for nw in (2, 4, 8)
        if (mt, nt, nw) != (4, 2, 8)]


def _all_cfgs():
    from kubernetes_gpu_cluster_amd.ops import gemm
    return gemm._W4_CONFIGS


@pytest.mark.parametrize("cfg", CFGS, ids=_cfg_id)
def test_w4_gemm_every_configuration(gpu, cfg):
    """Every built configuration against the fp32 CPU oracle and against the library GEMM on
    the widened weight (both multiply the same exact operand values).  K: the smallest the
    configuration takes (remainder units only), and 1664 per wave: 3 / 6 / 12 double-buffered
    batches at mt = 1 / 2 / 4 (a register set holds 4 / mt units; only 3 can be odd: the others
    are multiples of 2 by construction) plus one remainder unit.  N: one workgroup and three.
    M: 1, one that is no multiple of 16, 16 mt - 1 and 16 mt."""
    from kubernetes_gpu_cluster_amd.ops import gemm
    assert CFGS == _all_cfgs() and len(CFGS) == 17
    mt, nt, nw = cfg
    ms = sorted({1, 16 * mt - 9, 16 * mt - 1, 16 * mt})
    worst = 0.0
    for dt in DT:
        for K in (128 * nw, 1664 * nw):
            for N in (16 * nt, 48 * nt):
                w4, sc, dq = _weight(N, K, dt, gpu, seed=K + N)
                xs = _x(16 * mt, K, dt, gpu)
                exp = _oracle(xs, dq)
                wide = gemm.w4_widen(w4, sc, dt)
                assert torch.equal(wide.cpu().float(), dq)
                for M in ms:
                    assert gemm.w4_ok(M, N, K, cfg)
                    x = xs[:M]
                    got = gemm.w4_gemm(x, w4, sc, None, cfg).float().cpu()
                    worst = max(worst, ((got - exp[:M]).abs()
                                        / (TOL["atol"] + TOL["rtol"] * exp[:M].abs())).max().item())
                    torch.testing.assert_close(got, exp[:M], **TOL)
                    lib = torch.nn.functional.linear(x, wide).float().cpu()
                    torch.testing.assert_close(got, lib, **TOL)
                    assert torch.isfinite(got).all()
    print(f"K9f {cfg}: worst error / tolerance {worst:.3f}")


def test_w4_gemm_zero_block_contributes_nothing(gpu):
    """A weight that is zero except one block: the output is that block's dot product."""
    from kubernetes_gpu_cluster_amd.ops import gemm
    N, K = 32, 1024
    w = torch.zeros(N, K)
    w[:, 96:128] = torch.randn(N, 32, generator=torch.Generator().manual_seed(4))
    codes, scales = quantize_mxfp4(w.to(torch.bfloat16))
    dq = dequantize_mxfp4(codes, scales)
    x = _x(5, K, torch.bfloat16, gpu)
    for cfg in ((1, 1, 2), (1, 2, 4), (1, 1, 8)):
        got = gemm.w4_gemm(x, codes.to(gpu), scales.to(gpu), None, cfg).float().cpu()
        torch.testing.assert_close(got, x.float().cpu()[:, 96:128] @ dq[:, 96:128].t(), **TOL)


@pytest.mark.parametrize("dt", DT)
def test_w4_gemm_bias_strided_x_and_guard_rows(gpu, dt):
    from kubernetes_gpu_cluster_amd.ops import gemm
    N, K, M = 96, 1664 * 2, 21
    w4, sc, dq = _weight(N, K, dt, gpu, seed=7)
    big = _x(M, K + 1024, dt, gpu)
    x = big[:, 512:512 + K]                               # ldx > K, 16-byte aligned rows
    assert x.stride(0) > K and not x.is_contiguous()
    b = torch.randn(N, generator=torch.Generator().manual_seed(2)).to(dt).to(gpu)
    exp = _oracle(x, dq)
    for cfg in ((2, 1, 2), (2, 2, 2), (4, 1, 2)):
        torch.testing.assert_close(gemm.w4_gemm(x, w4, sc, None, cfg).float().cpu(), exp, **TOL)
        torch.testing.assert_close(gemm.w4_gemm(x, w4, sc, b, cfg).float().cpu(),
                                   exp + b.float().cpu(), **TOL)
        # rows of C beyond M keep their sentinel
        c = torch.full((M + 11, N), 512.0, dtype=dt, device=gpu)
        gemm.w4_gemm(x, w4, sc, b, cfg, c[:M])
        torch.testing.assert_close(c[:M].float().cpu(), exp + b.float().cpu(), **TOL)
        assert bool((c[M:] == 512.0).all())
    torch.testing.assert_close(gemm.linear(x, w4, b).float().cpu(), exp + b.float().cpu(), **TOL)


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("I", [16, 48])
def test_w4_silu_pairs_gate_and_up_rows(gpu, dt, I):
    """K9f's SiLU form over a merged [gate; up] weight [2I, K]: column g pairs gate row g with
    up row I + g; every nt = 2 configuration; and linear_silu takes it for an mxfp4 weight."""
    from kubernetes_gpu_cluster_amd.ops import gemm
    K = 1664 * 8                    # every nw: whole steps plus a remainder unit per wave
    w4, sc, dq = _weight(2 * I, K, dt, gpu, seed=I, spread=2)
    cfgs = [c for c in gemm._W4_CONFIGS if c[1] == 2 and gemm.w4_ok(16 * c[0], 2 * I, K, c)]
    assert len(cfgs) == 8
    for cfg in cfgs:
        for M in sorted({1, 16 * cfg[0] - 3, 16 * cfg[0]}):
            x = _x(M, K, dt, gpu, seed=M)
            ref = _oracle(x, dq)
            exp = torch.nn.functional.silu(ref[:, :I]) * ref[:, I:]
            out = torch.full((M + 2, I), float("nan"), dtype=dt, device=gpu)
            gemm.w4_silu(x, w4, sc, cfg, out[:M])
            torch.testing.assert_close(out[:M].float().cpu(), exp, **TOL)
            assert bool(out[M:].isnan().all())
    x = _x(5, K, dt, gpu)
    ref = _oracle(x, dq)
    before = gemm.w4_counts()["k9f_silu"]
    torch.testing.assert_close(gemm.linear_silu(x, w4).float().cpu(),
                               torch.nn.functional.silu(ref[:, :I]) * ref[:, I:], **TOL)
    assert gemm.w4_counts()["k9f_silu"] == before + 1


def test_bindings_reject_what_the_kernel_cannot_run(gpu):
    from kubernetes_gpu_cluster_amd.ops import _k, gemm
    dt = torch.bfloat16
    N, K = 64, 1024
    w4, sc, _ = _weight(N, K, dt, gpu)
    x = _x(16, K, dt, gpu)
    out = torch.empty(16, N, dtype=dt, device=gpu)
    k = _k()
    k.w4_gemm(out, x, w4, sc, None, 1, 1, 4, False)            # the valid call
    bad = [
        lambda: k.w4_gemm(out, x.float(), w4, sc, None, 1, 1, 4, False),            # X dtype
        lambda: k.w4_gemm(out.half(), x, w4, sc, None, 1, 1, 4, False),             # C dtype
        lambda: k.w4_gemm(out, x, w4.view(torch.int8), sc, None, 1, 1, 4, False),   # W4 dtype
        lambda: k.w4_gemm(out, x, w4, sc.float(), None, 1, 1, 4, False),            # scales dtype
        lambda: k.w4_gemm(out, x, w4, sc[:, :-1].contiguous(), None, 1, 1, 4, False),
        lambda: k.w4_gemm(out, x, w4, sc.t().contiguous(), None, 1, 1, 4, False),
        lambda: k.w4_gemm(out, x, w4, sc.flatten(), None, 1, 1, 4, False),
        lambda: k.w4_gemm(out, x, w4[:, 1:], sc, None, 1, 1, 4, False),             # not contiguous
        lambda: k.w4_gemm(out, x, w4, sc, None, 1, 1, 16, False),                   # nw
        lambda: k.w4_gemm(out, x, w4, sc, None, 3, 1, 4, False),                    # mt
        lambda: k.w4_gemm(out, x, w4, sc, None, 4, 2, 8, False),                    # not built
        lambda: k.w4_gemm(out, x, w4, sc, None, 1, 1, 4, True),                     # silu: nt = 2
        lambda: k.w4_gemm(out, x, w4, sc, None, 1, 2, 4, True),                     # silu: C [M, N/2]
        lambda: k.w4_gemm(out, x, w4, sc, torch.zeros(N - 1, dtype=dt, device=gpu), 1, 1, 4, False),
        lambda: k.w4_gemm(torch.empty(17, N, dtype=dt, device=gpu), _x(17, K, dt, gpu), w4, sc,
                          None, 1, 1, 4, False),                                     # M > 16 mt
        lambda: k.w4_gemm(out, _x(16, K + 8, dt, gpu)[:, 4:K + 4], w4, sc, None, 1, 1, 4, False),
        lambda: k.w4_gemm(torch.empty(16, 48, dtype=dt, device=gpu), x, w4[:48], sc[:48], None,
                          1, 2, 4, False),                                           # N % (16 nt)
        lambda: k.w4_widen(torch.empty(N, K, dtype=torch.float32, device=gpu), w4, sc),
        lambda: k.w4_widen(torch.empty(N, K // 2, dtype=dt, device=gpu), w4, sc),
        lambda: k.w4_widen(torch.empty(N, K, dtype=dt, device=gpu), w4, sc[:, :-1].contiguous()),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(RuntimeError):
            f()
            pytest.fail(f"call {i} was accepted")
    # K % (128 nw): rejected by the binding, refused by w4_ok, and the dispatcher widens
    w5, s5, dq5 = _weight(N, 1024 + 128, dt, gpu)
    x5 = _x(3, 1024 + 128, dt, gpu)
    assert not gemm.w4_ok(3, N, 1024 + 128, (1, 1, 2))
    with pytest.raises(RuntimeError, match="w4_gemm"):
        gemm.w4_gemm(x5, w5, s5, None, (1, 1, 2))
    assert not gemm.w4_ok(17, N, K, (1, 1, 4)) and not gemm.w4_ok(1, 16, K, (1, 2, 4))
    assert not gemm.w4_ok(64, N, 4096, (4, 2, 8)) and gemm.w4_ok(64, N, 4096, (4, 1, 8))
    assert gemm.w4_default_cfg(3, N, 1024 + 128) is None
    before = gemm.w4_counts()["widen"]
    torch.testing.assert_close(gemm.linear(x5, w5).float().cpu(), _oracle(x5, dq5), **TOL)
    assert gemm.w4_counts()["widen"] == before + 1


def test_configurations_cover_the_model_shapes():
    from kubernetes_gpu_cluster_amd.ops import gemm
    for K in (256, 512, 4096, 14336, 8192, 28672, 4096 // 8, 14336 // 8, 8192 // 8, 28672 // 8):
        for M in (1, 16, 17, 33, 64):
            assert any(gemm.w4_ok(M, 256, K, c) for c in gemm._W4_CONFIGS), (M, K)
            assert gemm.w4_default_cfg(M, 256, K) is not None, (M, K)
            assert gemm.w4_default_cfg(M, 256, K, silu=True)[1] == 2


# ------------------------------------------------------------------ dispatcher
def test_dispatcher_routes(gpu, monkeypatch):
    from kubernetes_gpu_cluster_amd.ops import gemm
    dt = torch.bfloat16
    N, K = 64, 1024
    w4, sc, dq = _weight(N, K, dt, gpu)
    x = _x(8, K, dt, gpu)
    exp = _oracle(x, dq)

    def moved(fn):
        a4, a8 = gemm.w4_counts(), gemm.w8_counts()
        y = fn()
        b4, b8 = gemm.w4_counts(), gemm.w8_counts()
        return y, {k: b4[k] - a4[k] for k in a4 if b4[k] != a4[k]}, \
            {k: b8[k] - a8[k] for k in a8 if b8[k] != a8[k]}

    try:
        gemm.clear_plan()
        y, d4, d8 = moved(lambda: gemm.linear(x, w4))           # no plan: the default cfg
        assert d4 == {"k9f": 1} and not d8
        torch.testing.assert_close(y.float().cpu(), exp, **TOL)
        gemm._plan_w4[(8, N, K)] = (1, 2, 2)
        y, d4, d8 = moved(lambda: gemm.linear_qkv(x, w4))       # the plan's configuration
        assert d4 == {"k9f": 1} and not d8
        torch.testing.assert_close(y.float().cpu(), exp, **TOL)
        gemm._plan_w4[(8, N, K)] = None                         # the tuner chose the widen path
        y, d4, d8 = moved(lambda: gemm.linear(x, w4))
        assert d4 == {"widen": 1} and not d8
        torch.testing.assert_close(y.float().cpu(), exp, **TOL)
        gemm._plan_w4_silu[(8, N, K)] = None
        y, d4, d8 = moved(lambda: gemm.linear_silu(x, w4))
        assert d4 == {"widen": 1} and not d8
        ref = torch.nn.functional.silu(exp[:, :N // 2]) * exp[:, N // 2:]
        torch.testing.assert_close(y.float().cpu(), ref, **TOL)
        gemm.clear_plan()
        assert not gemm.w4_plan() and not gemm.w4_silu_plan()
        x65 = _x(65, K, dt, gpu)
        y, d4, d8 = moved(lambda: gemm.linear(x65, w4))         # M = 65
        assert d4 == {"widen": 1} and not d8
        torch.testing.assert_close(y.float().cpu(), _oracle(x65, dq), **TOL)
        res = torch.zeros(8, N, dtype=dt, device=gpu)
        gam = torch.ones(N, dtype=dt, device=gpu)
        (_, r), d4, d8 = moved(lambda: gemm.linear_add_rms(x, w4, res, gam, 1e-5))
        assert d4 == {"k9f": 1} and not d8
        torch.testing.assert_close(r.float().cpu(), exp, **TOL)
        monkeypatch.setattr(gemm.W4, "enabled", False)          # KGC_W4_GEMM=0
        y, d4, d8 = moved(lambda: gemm.linear(x, w4))
        assert d4 == {"widen": 1} and not d8
        y, d4, d8 = moved(lambda: gemm.linear_silu(x, w4))
        assert d4 == {"widen": 1} and not d8
        monkeypatch.setattr(gemm.W4, "enabled", True)
        # fp8 and bf16 weights take their old routes
        w8, s8 = quantize_fp8_rows(torch.randn(N, K, dtype=dt, device=gpu) * K ** -0.5)
        _, d4, d8 = moved(lambda: gemm.linear(x, w8))
        assert not d4 and d8 == {"k9q": 1}
        _, d4, d8 = moved(lambda: gemm.linear(x65, w8))
        assert not d4 and d8 == {"widen": 1}
        wb = torch.randn(N, K, dtype=dt, device=gpu) * K ** -0.5
        y, d4, d8 = moved(lambda: gemm.linear(x, wb))
        assert not d4 and not d8
        torch.testing.assert_close(y.float().cpu(), x.float().cpu() @ wb.float().cpu().t(), **TOL)
    finally:
        gemm.clear_plan()


def test_tune_w4_writes_its_own_plans(gpu):
    from kubernetes_gpu_cluster_amd.ops import gemm
    dt = torch.bfloat16
    ws = [_weight(512, 1024, dt, gpu, seed=s)[0] for s in (1, 2)]
    try:
        gemm.clear_plan()
        res = gemm.tune_w4(ws, [4, 128], dt, silu_shapes={(512, 1024)}, reps=1)
        assert set(res) == {(4, 512, 1024)} and set(gemm.w4_plan()) == {(4, 512, 1024)}
        chosen, wide_us, best_us, best = res[(4, 512, 1024)]
        assert best in gemm._W4_CONFIGS and (chosen is None) == (best_us >= wide_us)
        assert set(gemm.w4_silu_plan()) == {(4, 512, 1024)}
        assert not gemm.w8_plan() and not gemm.plan()
        print("tune_w4:", res, gemm.w4_silu_plan())
    finally:
        gemm.clear_plan()


# ------------------------------------------------------------------ graph capture
def test_w4_paths_replay_in_a_graph(gpu):
    from kubernetes_gpu_cluster_amd.ops import gemm
    dt = torch.bfloat16
    N, K = 256, 2048
    w4, sc, dq = _weight(N, K, dt, gpu, seed=9, spread=2)
    xs = torch.zeros(8, K, dtype=dt, device=gpu)
    xl = torch.zeros(96, K, dtype=dt, device=gpu)
    gemm.clear_plan()
    gemm.w8_reserve(gpu, N * K, dt)               # static before capture
    for _ in range(2):
        gemm.linear(xs, w4)
        gemm.linear_silu(xs, w4)
        gemm.linear(xl, w4)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    c0 = gemm.w4_counts()
    with torch.cuda.graph(g):
        ys = gemm.linear(xs, w4)                  # K9f (default configuration)
        ya = gemm.linear_silu(xs, w4)             # its SiLU form
        yl = gemm.linear(xl, w4)                  # widen + library GEMM
    c1 = gemm.w4_counts()
    assert [c1[k] - c0[k] for k in ("k9f", "k9f_silu", "widen")] == [1, 1, 1]
    for seed in (1, 2):
        xs.copy_(_x(8, K, dt, gpu, seed=seed))
        xl.copy_(_x(96, K, dt, gpu, seed=seed + 10))
        g.replay()
        torch.cuda.synchronize()
        ref = _oracle(xs, dq)
        torch.testing.assert_close(ys.float().cpu(), ref, **TOL)
        torch.testing.assert_close(ya.float().cpu(), torch.nn.functional.silu(ref[:, :N // 2])
                                   * ref[:, N // 2:], **TOL)
        torch.testing.assert_close(yl.float().cpu(), _oracle(xl, dq), **TOL)


# ------------------------------------------------------------------ engine
@pytest.mark.parametrize("name", ["tiny-llama", "tiny-qwen2"])
def test_quantized_engine_graph_equals_eager(gpu, name):
    """Graph and eager engines run the same kernels (K9f at M <= 64, the widen path above):
    they agree on the first four tokens of every request."""
    from kubernetes_gpu_cluster_amd.engine.config import EngineConfig
    from kubernetes_gpu_cluster_amd.engine.llm_engine import LLMEngine
    from kubernetes_gpu_cluster_amd.engine.sequence import SamplingParams
    from kubernetes_gpu_cluster_amd.models.quant import dense_projections
    from kubernetes_gpu_cluster_amd.ops import gemm
    from kubernetes_gpu_cluster_amd.ops.quant import is_mxfp4
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(3, 1000, (n,), generator=g).tolist() for n in (5, 77, 300, 1)]
    params = [SamplingParams(temperature=1.0, seed=i, max_tokens=12, ignore_eos=True)
              for i in range(len(prompts))]
    outs = {}
    try:
        for eager in (True, False):
            gemm.clear_plan()
            eng = LLMEngine(EngineConfig(model=name, random_init=True, max_model_len=1024,
                                         max_num_seqs=16, max_num_batched_tokens=2048,
                                         num_gpu_blocks_override=512, cuda_graph_max_bs=16,
                                         enforce_eager=eager, quantization="mxfp4"))
            model = eng.executor.runner.model
            assert model.quantization == "mxfp4"
            assert all(is_mxfp4(m.weight) for l in model.layers for m in dense_projections(l))
            assert not gemm.w8_plan() and not gemm.w8_dg_plan()
            c0 = gemm.w4_counts()
            seqs = [eng.add_request(p, sp) for p, sp in zip(prompts, params)]
            while eng.has_unfinished():
                eng.step()
            outs[eager] = [s.output_token_ids for s in seqs]
            c1 = gemm.w4_counts()
            assert c1["widen"] > c0["widen"]                 # prefill of the 77 / 300 prompts
            if eager:
                assert c1["k9f"] > c0["k9f"] and c1["k9f_silu"] > c0["k9f_silu"]
            else:
                assert eng.executor.runner.stats["graph_steps"] > 0
                plan = gemm.w4_plan()
                assert plan and all(M <= 16 for M, _, _ in plan)
                print(name, "plan:", plan, gemm.w4_silu_plan())
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
                             num_gpu_blocks_override=512, cuda_graph_max_bs=2,
                             quantization="mxfp4"))
g = torch.Generator().manual_seed(1)
seqs = [eng.add_request(torch.randint(100, 128000, (n,), generator=g).tolist(),
                        SamplingParams(temperature=1.0, seed=n, max_tokens=6, ignore_eos=True))
        for n in (5, 300)]
while eng.has_unfinished():
    eng.step()
ops.debug_check()
assert all(len(s.output_token_ids) == 6 for s in seqs)
assert eng.executor.runner.stats["graph_steps"] > 0
c = gemm.w4_counts()
assert c["k9f"] > 0 and c["k9f_silu"] > 0 and c["widen"] > 0, c
plan = gemm.w4_plan()
assert plan and any(v is not None for v in plan.values()), plan
print("W4-DEBUG-BUILD-OK", c, plan, gemm.w4_silu_plan())
'''


def test_quantized_engine_in_the_debug_build(gpu):
    """The mxfp4 engine on Llama-3-8B's shapes (prefill through the widen path, tuned and
    graphed K9f decode) on the bounds-checking library, in a child process: one process
    cannot load both builds."""
    so = os.path.join(ROOT, "kubernetes_gpu_cluster_amd", "_kgc_ops_debug.so")
    if not os.path.exists(so):
        pytest.fail("debug build missing: run KGC_HIP_DEBUG=1 python csrc/build.py")
    pp = os.environ.get("PYTHONPATH", "")
    env = dict(os.environ, KGC_HIP_DEBUG="1",
               PYTHONPATH=os.pathsep.join([p for p in pp.split(os.pathsep) if p] + [ROOT]))
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "W4-DEBUG-BUILD-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
