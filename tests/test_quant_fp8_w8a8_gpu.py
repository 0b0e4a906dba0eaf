"""K9a (csrc/kernels/gemm_w8a8.hip): the quantiser against quantize_fp8_rows bit for bit, the
GEMM against float64 on the codes and scales it was given, routing, graph replay, the engine."""
import pytest
import torch

from kubernetes_gpu_cluster_amd.ops import gemm
from kubernetes_gpu_cluster_amd.ops.quant import mark_act_fp8, quantize_fp8_rows

pytestmark = pytest.mark.gpu
DT = [torch.bfloat16, torch.float16]
A8 = gemm.W8A8
NCFG = lambda: int(torch.ops.kgc.w8a8_gemm_num_cfgs())  # noqa: E731


def _rows(M, K, dt, gpu):                     # magnitudes 2^-10 .. 2^10, then the special rows
    g =torch.Generator(device=gpu).manual_seed(M + K)
    x = torch.randn(M, K, device=gpu, generator=g) * (2.0 ** (torch.arange(M, device=gpu) % 21 - 10))[:, None]
    x = x.to(dt)
    x[0, 5] = -0.0
    if M > 3:
        x[1] = 0                                   # scale 1, codes 0
        x[2] = (torch.randn(K, device=gpu, generator=g) * 2.0 ** -3).to(dt)
        x[2, 7] = -(2.0 ** 9)                      # lands on -448, its neighbours subnormal
        x[3, ::2] = -0.0
    return x


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("K", [128, 384, 4096])
@pytest.mark.parametrize("M", [1, 65, 300])
def test_act_quant_is_quantize_fp8_rows(gpu, dt, M, K, strided):
    x = _rows(M, K, dt, gpu)
    if strided:
        x = torch.cat([x, x, x[:, :8]], dim=1)[:, K:2 * K]      # row stride 2 K + 8
    xq = torch.empty(M, K, dtype=torch.float8_e4m3fn, device=gpu)
    xs = torch.empty(M, dtype=torch.float32, device=gpu)
    torch.ops.kgc.act_quant_fp8(xq, xs, x)
    eq, es = quantize_fp8_rows(x.cpu())
    assert torch.equal(xs.cpu(), es)
    assert torch.equal(xq.cpu().view(torch.uint8), eq.view(torch.uint8))
    if M > 3:
        assert es[1] == 1.0 and not eq[1].view(torch.uint8).any() and eq[2, 7].float() == -448.0


_cases: dict = {}
SHAPES = [(65, 128, 128), (129, 384, 384), (257, 128, 2048), (300, 384, 2048), (1, 128, 128)]


def _case(gpu, dt, M, N, K):
    """(xq, xs, w8, ws, bias, float64 oracle without bias, error bound), made once per shape."""
    key = (dt, M, N, K)
    if key not in _cases:
        g = torch.Generator(device=gpu).manual_seed(M * 7 + N + K)
        x = torch.randn(M, K, device=gpu, generator=g) * (2.0 ** (torch.arange(M, device=gpu) % 13 - 6))[:, None]
        w = torch.randn(N, K, device=gpu, generator=g) * K ** -0.5
        w[N // 2:] *= 4
        xq, xs = quantize_fp8_rows(x.to(dt))
        w8, ws = quantize_fp8_rows(w.to(dt))
        b = torch.randn(N, device=gpu, generator=g).to(dt)
        xd, wd = xq.double().cpu(), w8.double().cpu()
        sx, sw = xs.double().cpu()[:, None], ws.double().cpu()[None, :]
        exp = (xd @ wd.t()) * sx * sw
        acc = K * 2.0 ** -23 * (xd.abs() @ wd.abs().t()) * sx * sw
        _cases[key] = (xq, xs, w8, ws, b, exp, acc)
    return _cases[key]


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_w8a8_gemm_every_cfg_against_float64(gpu, dt, M, N, K):
    xq, xs, w8, ws, b, exp, acc = _case(gpu, dt, M, N, K)
    worst, first = 0.0, {}
    for cfg in range(NCFG()):
        for bias in (None, b):
            e = exp if bias is None else exp + bias.double().cpu()
            buf = torch.full((M + 8, N), float("nan"), dtype=dt, device=gpu)
            torch.ops.kgc.w8a8_gemm(buf[:M], xq, xs, w8, ws, bias, cfg)
            assert bool(torch.isnan(buf[M:]).all())
            got = buf[:M].cpu()
            ratio = ((got.double() - e).abs() / (2.0 ** -8 * e.abs() + acc)).nan_to_num(nan=float("inf"))
            worst = max(worst, ratio.max().item())
            assert torch.equal(first.setdefault(bias is None, got).view(torch.int16),
                               got.view(torch.int16)), f"cfg {cfg} differs from cfg 0"
    print(f"K9a {dt} M={M} N={N} K={K}: {NCFG()} cfgs, worst error / bound {worst:.3f}")
    assert worst <= 1.0


def test_cfg_table_and_refusals(gpu):
    k = torch.ops.kgc
    tiles = [tuple(k.w8a8_gemm_cfg_info(c)) for c in range(NCFG())]
    assert {(256, 128), (256, 256), (128, 128)} <= {t[:2] for t in tiles}
    with pytest.raises(RuntimeError, match="tile config"):
        k.w8a8_gemm_cfg_info(NCFG())
    for M, N, K, cfg, odt in [(65, 192, 128, 0, DT[0]), (65, 128, 192, 0, DT[0]),
                              (65, 128, 128, NCFG(), DT[0]), (65, 128, 128, 0, torch.float32)]:
        xq, xs = quantize_fp8_rows(torch.randn(M, K, device=gpu))
        w8, ws = quantize_fp8_rows(torch.randn(N, K, device=gpu))
        out = torch.full((M, N), 7.0, dtype=odt, device=gpu)
        with pytest.raises(RuntimeError, match="w8a8_gemm"):
            k.w8a8_gemm(out, xq, xs, w8, ws, None, cfg)
        assert bool((out == 7.0).all())


def _oracle(x, w8, ws, a8):                   # a8: of the per-token quantised x
    xq, xs = quantize_fp8_rows(x.cpu())
    xd = xq.double() * xs.double()[:, None] if a8 else x.double().cpu()
    return xd @ (w8.double().cpu() * ws.double().cpu()[:, None]).t()


@pytest.mark.parametrize("dt", DT)
def test_routing(gpu, dt):
    tol = dict(atol=3e-2, rtol=2e-2)           # test_quant_fp8_gpu.py's, for the W8A16 paths
    g = torch.Generator(device=gpu).manual_seed(2)
    x = torch.randn(300, 512, device=gpu, generator=g).to(dt)
    w = (torch.randn(384, 512, device=gpu, generator=g) * 512 ** -0.5).to(dt)
    plain, ws = quantize_fp8_rows(w)
    marked = mark_act_fp8(quantize_fp8_rows(w)[0])
    odd = mark_act_fp8(quantize_fp8_rows(w[:, :192])[0])
    gemm.clear_plan()

    def run(x, w8, q, key, **tol):
        c0, w0 = dict(q.counts), dict(gemm.W8.counts)
        got = gemm.linear(x, w8).double().cpu()
        assert q.counts[key] == c0[key] + 1 and sum(q.counts.values()) == sum(c0.values()) + 1
        assert q is gemm.W8 or gemm.W8.counts == w0
        torch.testing.assert_close(got, _oracle(x, w8, w8.w8_scale, key == "k9a"), **tol)
    # one bf16 / f16 rounding of an fp32 sum of 512 exact products: 2^-8 and change
    run(x, marked, A8, "k9a", atol=1e-3, rtol=2.0 ** -7)
    run(x[:16], marked, A8, "k9q", **tol)
    run(x[:, :192], odd, A8, "widen", **tol)
    run(x, plain, gemm.W8, "widen", **tol)
    A8.a8_enabled = False
    try:
        run(x, marked, A8, "widen", **tol)
    finally:
        A8.a8_enabled = True


def test_linear_replays_in_a_graph(gpu):
    g = torch.Generator(device=gpu).manual_seed(3)
    w8 = mark_act_fp8(quantize_fp8_rows((torch.randn(384, 512, device=gpu, generator=g) * 0.05).bfloat16())[0])
    x = torch.zeros(300, 512, dtype=torch.bfloat16, device=gpu)
    gemm.clear_plan()
    gemm.linear(x, w8)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    c0 = A8.counts["k9a"]
    with torch.cuda.graph(graph):
        y = gemm.linear(x, w8)
    assert A8.counts["k9a"] == c0 + 1
    for seed in (1, 2):
        x.copy_(torch.randn(x.shape, device=gpu, generator=g.manual_seed(seed)))
        graph.replay()
        torch.cuda.synchronize()
        got = y.clone()
        assert bool(got.any()) and torch.equal(got, gemm.linear(x, w8))


def test_engine_prefills_on_k9a(gpu):
    from kubernetes_gpu_cluster_amd.engine.sequence import SamplingParams
    from test_engine_gpu import _run, _tiny_engine
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(100, 128000, (n,), generator=g).tolist() for n in (70, 133, 200, 96)]
    params = [SamplingParams(temperature=1.0, seed=i, max_tokens=6, ignore_eos=True)
              for i in range(len(prompts))]
    outs = {}
    for name, method, eager in (("graph", "fp8_w8a8", False), ("eager", "fp8_w8a8", True),
                                ("fp8", "fp8", False)):
        gemm.clear_plan()
        c0 = A8.counts["k9a"]
        eng = _tiny_engine(enforce_eager=eager, quantization=method)
        outs[name] = _run(eng, prompts, params)
        assert (A8.counts["k9a"] > c0) == (method == "fp8_w8a8")
        del eng
        torch.cuda.empty_cache()
    gemm.clear_plan()
    assert all(len(o) == 6 for v in outs.values() for o in v)
    for a, b in zip(outs["graph"], outs["eager"]):
        assert a[:4] == b[:4], (a, b)
    same = sum(a[0] == b[0] for a, b in zip(outs["graph"], outs["fp8"]))
    print(f"first tokens, fp8_w8a8 vs fp8: {same} / {len(prompts)} agree")
