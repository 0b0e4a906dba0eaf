"""K9mf on the MI355X (csrc/kernels/gemm_w4_decode.hip): the K9m pipeline over packed mxfp4
weights at 64 < M <= 512, against the fp32 CPU oracle of test_quant_mxfp4_gpu.py (the same
codes and scales through ``dequantize_mxfp4``), its tolerance, weights and inputs; the
dispatcher, graph replay and the quantised engine at a decode bucket above 64."""
import faulthandler
import os
import subprocess
import sys

import pytest
import torch

from kubernetes_gpu_cluster_amd.ops.quant import (MXFP4_TILE_BYTES, attach_w4_scale,
                                                  dequantize_mxfp4, pack_mxfp4_tiles_reference,
                                                  quantize_mxfp4)
from test_quant_mxfp4_gpu import _weight, _x

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DT = [torch.bfloat16, torch.float16]
TOL = dict(atol=3e-2, rtol=2e-2)       # the project's (test_quant_mxfp4_gpu.py)
PARTIAL, OUT, SILU = 0, 1, 2


@pytest.fixture(autouse=True)
def _time_limit():
    """Each test's GPU work runs under its own time limit: a hung kernel ends the process
    (with a traceback) instead of holding the card."""
    faulthandler.dump_traceback_later(240, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _oracle(x, dq):
    return x.float().cpu() @ dq.t()


def _pack(w4, sc, silu):
    N, K = w4.shape[0], 2 * w4.shape[1]
    p = torch.empty(N // 128, K // 64, MXFP4_TILE_BYTES, dtype=torch.uint8, device=w4.device)
    torch.ops.kgc.w4_dgemm_pack(p, w4, sc, silu)
    return p


def _tile_bytes(N, K):
    return N // 128 * (K // 64) * MXFP4_TILE_BYTES


_cases: dict = {}


def _case(gpu, dt, M, N, K):
    """(x, w4, scales, packed, oracle) on test_quant_mxfp4_gpu's weight (block kb of row n on
    the scale 2^((kb + 3 n) % 19 - 9), one zero block), made once per shape and shared."""
    key = (dt, M, N, K)
    if key not in _cases:
        if K < 128:
            # _weight wants three distinct scales in a row: the first K columns of a 256-wide
            # one (the same blocks on the same scales, the zero block among them)
            w4, sc, dq = _weight(N, 256, dt, gpu, seed=N + K)
            sc, dq = sc[:, :K // 32].contiguous(), dq[:, :K].contiguous()
            w4 = attach_w4_scale(w4[:, :K // 2].contiguous(), sc)
        else:
            w4, sc, dq = _weight(N, K, dt, gpu, seed=N + K)
        x = _x(M, K, dt, gpu, seed=M)
        _cases[key] = (x, w4, sc, _pack(w4, sc, False), _oracle(x, dq))
    return _cases[key]


def _ncfg():
    return int(torch.ops.kgc.w4_dgemm_num_cfgs())


def test_cfg_table(gpu):
    tiles = [tuple(torch.ops.kgc.w4_dgemm_cfg_info(c)) for c in range(_ncfg())]
    assert {(256, 128, 3), (256, 128, 4), (128, 128, 3), (128, 128, 4), (128, 128, 6)} <= set(tiles)
    with pytest.raises(RuntimeError, match="tile config"):
        torch.ops.kgc.w4_dgemm_cfg_info(_ncfg())


@pytest.mark.parametrize("silu", [False, True])
def test_pack_kernel_matches_the_reference(gpu, silu):
    w4, sc = quantize_mxfp4(torch.randn(256, 192) * 192 ** -0.5)
    got = _pack(w4.to(gpu), sc.to(gpu), silu).cpu()
    assert torch.equal(got, pack_mxfp4_tiles_reference(w4, sc, silu))


# K9mq's shapes.  M: one row into a block / into the second block / exact blocks / a ragged
# last block of a 256-row tile; N: one tile / an odd tile count; K: one step (shorter than
# the ring's prologue) / three (no walk rotation) / 16 (rotated); S = 3 at K = 1024: uneven
# slices
SHAPES = [(65, 128, 64, (1,)), (129, 384, 192, (1, 2, 3)), (256, 128, 1024, (1, 2)),
          (300, 384, 1024, (1, 3)), (65, 384, 1024, (2,))]


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("M,N,K,splits", SHAPES)
def test_w4_dgemm_every_cfg(gpu, dt, M, N, K, splits):
    k = torch.ops.kgc
    x, w4, sc, wp, exp = _case(gpu, dt, M, N, K)
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
                k.w4_dgemm(out, x, wp, None, cfg, OUT)
                got = out.float().cpu()
                worst = max(worst, ((got - exp).abs() / (TOL["atol"] + TOL["rtol"] * exp.abs())).max().item())
                torch.testing.assert_close(got, exp, **TOL)
                out.fill_(float("nan"))
                k.w4_dgemm(out, x, wp, b, cfg, OUT)
                torch.testing.assert_close(out.float().cpu(), exp + b.float().cpu(), **TOL)
                continue
            ws = torch.full((S, M, N), float("nan"), dtype=torch.float32, device=gpu)
            k.w4_dgemm(ws, x, wp, None, cfg, PARTIAL)
            got = ws.sum(0).cpu()
            worst = max(worst, ((got - exp).abs() / (TOL["atol"] + TOL["rtol"] * exp.abs())).max().item())
            torch.testing.assert_close(got, exp, **TOL)
            red = torch.empty(M, N, dtype=dt, device=gpu)
            k.splitk_reduce(red, ws)
            torch.testing.assert_close(red.float().cpu(), exp, **TOL)
            res = res0.clone()
            k.splitk_add_rms_norm(red, ws, res, gamma, 1e-6)
            torch.testing.assert_close(res.float().cpu(), rn, **TOL)
            torch.testing.assert_close(red.float().cpu(), norm, **TOL)
    print(f"K9mf {dt} M={M} N={N} K={K}: {_ncfg()} cfgs, worst error / tolerance {worst:.3f}")


def test_w4_dgemm_rejects_what_it_cannot_run(gpu):
    k = torch.ops.kgc
    dt = torch.bfloat16
    x, w4, sc, wp, _ = _case(gpu, dt, 65, 128, 64)
    out = torch.empty(65, 128, dtype=dt, device=gpu)
    with pytest.raises(RuntimeError, match="tile config"):
        k.w4_dgemm(out, x, wp, None, _ncfg(), OUT)
    with pytest.raises(RuntimeError, match="tile config"):
        k.w4_dgemm(out, x, wp, None, -1, OUT)
    with pytest.raises(RuntimeError, match="64 < M"):
        k.w4_dgemm(out[:64], x[:64], wp, None, 0, OUT)
    with pytest.raises(RuntimeError, match="K / 64"):
        k.w4_dgemm(torch.empty(2, 65, 128, device=gpu), x, wp, None, 0, PARTIAL)
    with pytest.raises(RuntimeError, match="no bias"):
        k.w4_dgemm(torch.empty(1, 65, 128, device=gpu), x, wp, out[0], 0, PARTIAL)
    with pytest.raises(RuntimeError, match="X"):
        k.w4_dgemm(out, x.to(torch.float16), wp, None, 0, OUT)
    with pytest.raises(RuntimeError, match="X"):
        k.w4_dgemm(out, x.float(), wp, None, 0, OUT)
    with pytest.raises(RuntimeError, match="packed Wp"):
        k.w4_dgemm(out, x, wp[:, :, :4096].contiguous(), None, 0, OUT)
    with pytest.raises(RuntimeError, match="silu"):
        k.w4_dgemm(torch.empty(65, 64, dtype=dt, device=gpu), x, wp, out[0], 0, SILU)
    with pytest.raises(RuntimeError, match="C \\[M, N\\]"):
        k.w4_dgemm(out, x, wp, None, 0, SILU)                  # SiLU pairs are [M, N / 2]


@pytest.mark.parametrize("dt", DT)
def test_guard_rows_stay_untouched(gpu, dt):
    """out is the first M rows of a NaN-filled [M + 3, N] buffer: rows >= M are never stored."""
    k = torch.ops.kgc
    M, N, K = 129, 256, 192
    x, w4, sc, wp, _ = _case(gpu, dt, M, N, K)
    wps = _pack(w4, sc, True)
    for cfg in range(_ncfg()):
        buf = torch.full((M + 3, N), float("nan"), dtype=dt, device=gpu)
        k.w4_dgemm(buf[:M], x, wp, None, cfg, OUT)
        assert bool(torch.isfinite(buf[:M]).all()) and bool(torch.isnan(buf[M:]).all())
        buf = torch.full((M + 3, N // 2), float("nan"), dtype=dt, device=gpu)
        k.w4_dgemm(buf[:M], x, wps, None, cfg, SILU)
        assert bool(torch.isfinite(buf[:M]).all()) and bool(torch.isnan(buf[M:]).all())


def test_zero_block_and_zero_row(gpu):
    """_weight's zero block (block 1 of row 2) and one all-zero row: the row's outputs, and
    its slices, are exact zeros (a scale or a code taken from a neighbour would not be)."""
    k = torch.ops.kgc
    dt = torch.bfloat16
    M, N, K = 80, 384, 1024
    w4, sc, dq = _weight(N, K, dt, gpu, seed=11)
    assert bool((dq[2, 32:64] == 0).all()) and bool((dq[2] != 0).any())
    w4 = w4.clone()
    w4[37] = 0                                     # +0 codes: the whole row is zero
    attach_w4_scale(w4, sc)
    dq = dequantize_mxfp4(w4.cpu(), sc.cpu())
    assert bool((dq[37] == 0).all())
    x = _x(M, K, dt, gpu)
    exp = _oracle(x, dq)
    wp = _pack(w4, sc, False)
    for cfg in range(_ncfg()):
        out = torch.empty(M, N, dtype=dt, device=gpu)
        k.w4_dgemm(out, x, wp, None, cfg, OUT)
        torch.testing.assert_close(out.float().cpu(), exp, **TOL)
        assert bool((out[:, 37] == 0).all())
        ws = torch.empty(2, M, N, dtype=torch.float32, device=gpu)
        k.w4_dgemm(ws, x, wp, None, cfg, PARTIAL)
        torch.testing.assert_close(ws.sum(0).cpu(), exp, **TOL)
        assert bool((ws[:, :, 37] == 0).all())
    # a row that is zero only in block 1: x restricted to that block gives exact zeros
    xz = torch.zeros_like(x)
    xz[:, 32:64] = x[:, 32:64]
    out = torch.empty(M, N, dtype=dt, device=gpu)
    k.w4_dgemm(out, xz, wp, None, 2, OUT)
    assert bool((out[:, 2] == 0).all()) and bool((out[:, 3] != 0).any())
    torch.testing.assert_close(out.float().cpu(), _oracle(xz, dq), **TOL)


def _silu_weight(I, K, dt, gpu):
    """A merged [gate; up] mxfp4 weight on _weight's scale pattern, the up rows x 4."""
    w4, sc, dq = _weight(2 * I, K, dt, gpu, seed=I)
    sc = sc.clone()
    sc[I:] += 2                                    # e8m0: two exponent steps = x 4
    attach_w4_scale(w4, sc)
    return w4, sc, dequantize_mxfp4(w4.cpu(), sc.cpu())


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("M,I", [(65, 128), (200, 256), (200, 128), (65, 256)])
def test_silu_form(gpu, dt, M, I):
    """The SiLU epilogue and the S = 2 slices + splitk_reduce_silu over a merged [gate; up]
    weight whose up rows sit on another scale; linear_silu takes an installed entry."""
    from kubernetes_gpu_cluster_amd.ops import gemm
    k = torch.ops.kgc
    N, K = 2 * I, 1024
    w4, sc, dq = _silu_weight(I, K, dt, gpu)
    x = _x(M, K, dt, gpu, seed=M)
    ref = _oracle(x, dq)
    exp = torch.nn.functional.silu(ref[:, :I]) * ref[:, I:]
    assert gemm.pack_w4_decode_weights([], [w4]) == _tile_bytes(N, K)
    for cfg in range(_ncfg()):
        got = gemm.w4_dgemm(x, w4, cfg, 1, epi=SILU)
        torch.testing.assert_close(got.float().cpu(), exp, **TOL)
        red = torch.empty(M, I, dtype=dt, device=gpu)
        k.splitk_reduce_silu(red, gemm.w4_dgemm(x, w4, cfg, 2, silu_w=True), True)
        torch.testing.assert_close(red.float().cpu(), exp, **TOL)
    try:
        for plan in ((0, 1), (_ncfg() - 1, 2)):
            gemm._plan_w4_dg[(M, N, K, "silu")] = plan
            before = gemm.w4_counts()["k9mf_silu"]
            torch.testing.assert_close(gemm.linear_silu(x, w4).float().cpu(), exp, **TOL)
            assert gemm.w4_counts()["k9mf_silu"] == before + 1
    finally:
        gemm.clear_plan()


def test_strided_x(gpu):
    """X may be a row-strided view: a [96, 1024] slice of a [96, 3072] buffer."""
    from kubernetes_gpu_cluster_amd.ops import gemm
    dt = torch.bfloat16
    big = _x(96, 3072, dt, gpu, seed=3)
    x = big[:, 1024:2048]
    w4, sc, dq = _weight(512, 1024, dt, gpu, seed=3)
    exp = _oracle(x, dq)
    assert gemm.pack_w4_decode_weights([w4], []) == _tile_bytes(512, 1024)
    for cfg in range(_ncfg()):
        torch.testing.assert_close(gemm.w4_dgemm(x, w4, cfg, 1).float().cpu(), exp, **TOL)
        ws = gemm.w4_dgemm(x, w4, cfg, 2)
        torch.testing.assert_close(ws.sum(0).cpu(), exp, **TOL)


def test_dispatcher_takes_the_plan_and_falls_back(gpu):
    from kubernetes_gpu_cluster_amd.ops import gemm
    dt = torch.bfloat16
    M, N, K = 96, 512, 1024
    x = _x(M, K, dt, gpu, seed=4)
    w4, sc, dq = _weight(N, K, dt, gpu, seed=4)
    b = torch.randn(N, dtype=dt, device=gpu)
    exp = _oracle(x, dq)
    gemm.clear_plan()
    try:
        # an entry, but no packed copy: the widen path
        gemm._plan_w4_dg[(M, N, K, "plain")] = (2, 1)
        c0 = gemm.w4_counts()
        torch.testing.assert_close(gemm.linear(x, w4).float().cpu(), exp, **TOL)
        c1 = gemm.w4_counts()
        assert c1["widen"] == c0["widen"] + 1 and c1["k9mf"] == c0["k9mf"]
        assert gemm.pack_w4_decode_weights([w4], []) == _tile_bytes(N, K)
        assert gemm.pack_w4_decode_weights([w4], []) == 0            # packed once
        assert torch.equal(gemm.w4_packed_weight(w4).cpu(),
                           pack_mxfp4_tiles_reference(w4.cpu(), sc.cpu()))
        torch.testing.assert_close(gemm.linear(x, w4).float().cpu(), exp, **TOL)
        torch.testing.assert_close(gemm.linear(x, w4, b).float().cpu(), exp + b.float().cpu(), **TOL)
        c2 = gemm.w4_counts()
        assert c2["k9mf"] == c1["k9mf"] + 2 and c2["widen"] == c1["widen"]
        # split-K: slices + splitk_reduce; with a bias, the widen path
        gemm._plan_w4_dg[(M, N, K, "plain")] = (3, 4)
        torch.testing.assert_close(gemm.linear(x, w4).float().cpu(), exp, **TOL)
        torch.testing.assert_close(gemm.linear(x, w4, b).float().cpu(), exp + b.float().cpu(), **TOL)
        c3 = gemm.w4_counts()
        assert c3["k9mf"] == c2["k9mf"] + 1 and c3["widen"] == c2["widen"] + 1
        # a None entry, another M, the knob off: the widen path
        gemm._plan_w4_dg[(M, N, K, "plain")] = None
        gemm.linear(x, w4)
        gemm._plan_w4_dg[(M, N, K, "plain")] = (2, 1)
        gemm.linear(x[:80], w4)
        mode, gemm.W4.dgemm_mode = gemm.W4.dgemm_mode, "0"
        try:
            gemm.linear(x, w4)
        finally:
            gemm.W4.dgemm_mode = mode
        c4 = gemm.w4_counts()
        assert c4["k9mf"] == c3["k9mf"] and c4["widen"] == c3["widen"] + 3
        gemm.clear_plan()
        torch.testing.assert_close(gemm.linear(x, w4).float().cpu(), exp, **TOL)
        c5 = gemm.w4_counts()
        assert c5["k9mf"] == c4["k9mf"] and c5["widen"] == c4["widen"] + 1
        assert c5["k9mf_silu"] == c0["k9mf_silu"] and c5["k9f"] == c0["k9f"]
    finally:
        gemm.clear_plan()


def test_tuner_plans_only_packed_weights(gpu):
    """tune_w4 never packs: an unpacked shape gets its M <= 64 entry only; once packed, force
    mode names a configuration per mid bucket and kind, in w4_dg_plan() and not in w4_plan()."""
    from kubernetes_gpu_cluster_amd.ops import gemm
    dt = torch.bfloat16
    w4, sc, _ = _weight(512, 1024, dt, gpu, seed=6)
    mode = gemm.W4.dgemm_mode
    gemm.clear_plan()
    try:
        gemm.W4.dgemm_mode = "force"
        res = gemm.tune_w4([w4], [4, 128], dt, reps=1)
        assert set(res) == {(4, 512, 1024)} and set(gemm.w4_plan()) == {(4, 512, 1024)}
        assert not gemm.w4_dg_plan() and gemm.w4_packed_weight(w4) is None
        gemm.pack_w4_decode_weights([w4], [])
        res = gemm.tune_w4([w4], [128, 300], dt, reps=1, tail_shapes={(512, 1024)})
        assert set(res) == {(128, 512, 1024, "tail"), (300, 512, 1024, "tail")}
        assert gemm.w4_dg_plan() == {k: v[0] for k, v in res.items()}
        assert set(gemm.w4_plan()) == {(4, 512, 1024)}
        assert gemm.tail_plan_has_m(128) and not gemm.tail_plan_has_m(4)
    finally:
        gemm.W4.dgemm_mode = mode
        gemm.clear_plan()


def test_paths_replay_in_a_graph(gpu):
    """linear, linear_silu and linear_add_rms at M = 96 with entries installed, captured and
    replayed on two fresh inputs."""
    from kubernetes_gpu_cluster_amd.ops import gemm
    dt = torch.bfloat16
    M, K, N, I = 96, 1024, 512, 256
    w4, _, dq = _weight(N, K, dt, gpu, seed=9)
    wo, _, dqo = _weight(N, K, dt, gpu, seed=10)
    wg, _, dqg = _silu_weight(I, K, dt, gpu)
    gamma = torch.rand(N, dtype=dt, device=gpu) + 0.5
    x = torch.zeros(M, K, dtype=dt, device=gpu)
    res = torch.zeros(M, N, dtype=dt, device=gpu)
    gemm.clear_plan()
    gemm.pack_w4_decode_weights([w4, wo], [wg])
    try:
        gemm._plan_w4_dg[(M, N, K, "plain")] = (2, 2)
        gemm._plan_w4_dg[(M, 2 * I, K, "silu")] = (3, 1)
        gemm._plan_w4_dg[(M, N, K, "tail")] = (4, 2)

        def body():
            return (gemm.linear(x, w4), gemm.linear_silu(x, wg),
                    gemm.linear_add_rms(x, wo, res, gamma, 1e-6)[0])
        c0 = gemm.w4_counts()
        body()
        c1 = gemm.w4_counts()
        assert (c1["k9mf"], c1["k9mf_silu"], c1["widen"]) == (c0["k9mf"] + 2, c0["k9mf_silu"] + 1,
                                                              c0["widen"])
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            y, a, nrm = body()
        for seed in (1, 2):
            x.copy_(_x(M, K, dt, gpu, seed=seed))
            gen = torch.Generator(device=gpu).manual_seed(seed)
            r0 = torch.randn(res.shape, device=gpu, generator=gen).to(dt)
            res.copy_(r0)
            g.replay()
            torch.cuda.synchronize()
            torch.testing.assert_close(y.float().cpu(), _oracle(x, dq), **TOL)
            gu = _oracle(x, dqg)
            torch.testing.assert_close(a.float().cpu(),
                                       torch.nn.functional.silu(gu[:, :I]) * gu[:, I:], **TOL)
            rn = r0.float().cpu() + _oracle(x, dqo)
            torch.testing.assert_close(res.float().cpu(), rn, **TOL)
            exp = rn * torch.rsqrt(rn.pow(2).mean(-1, keepdim=True) + 1e-6) * gamma.float().cpu()
            torch.testing.assert_close(nrm.float().cpu(), exp, **TOL)
    finally:
        gemm.clear_plan()


# ------------------------------------------------------------------ engine
def test_quantized_engine_at_a_mid_bucket(gpu):
    """80 sequences decode in the 80-row bucket: K9mf in force mode, graph against eager (both
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
    mode = gemm.W4.dgemm_mode
    try:
        for name, knob, eager in (("graph", "force", False), ("eager", "force", True),
                                  ("off", "0", False)):
            gemm.clear_plan()
            gemm.W4.dgemm_mode = knob
            c0 = gemm.w4_counts()      # (a graph engine's GEMM calls are counted at capture)
            eng = _tiny_engine(enforce_eager=eager, quantization="mxfp4", max_num_seqs=96,
                               cuda_graph_max_bs=128)
            outs[name] = _run(eng, prompts, params)
            c1 = gemm.w4_counts()
            layers = eng.executor.runner.model.layers
            packed = [gemm.w4_packed_weight(layers[0].self_attn.o_proj.weight),
                      gemm.w4_packed_weight(layers[0].mlp.gate_up_proj.weight, True)]
            if knob == "0":
                assert c1["k9mf"] == c0["k9mf"] and c1["k9mf_silu"] == c0["k9mf_silu"]
                assert not gemm.w4_dg_plan() and packed == [None, None]
            else:
                assert all(p is not None for p in packed)
                assert any(k[0] > 64 and v is not None for k, v in gemm.w4_dg_plan().items())
                assert c1["k9mf"] > c0["k9mf"] and c1["k9mf_silu"] > c0["k9mf_silu"]
            if not eager:
                assert eng.executor.runner.stats["graph_steps"] > 0
            del eng, layers, packed
            torch.cuda.empty_cache()
    finally:
        gemm.W4.dgemm_mode = mode
        gemm.clear_plan()
    assert all(len(o) == 6 for v in outs.values() for o in v)
    for a, b in zip(outs["graph"], outs["eager"]):
        assert a[:4] == b[:4], (a, b)
    same = sum(a[0] == b[0] for a, b in zip(outs["graph"], outs["off"]))
    print(f"first tokens, K9mf (force) vs the widen path: {same} / {len(prompts)} agree")


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
assert gemm.W4.dgemm_mode == "force"
PRESETS["llama-3-8b-2l"] = PRESETS["llama-3-8b"].shrink(name="llama-3-8b-2l", num_layers=2)
eng = LLMEngine(EngineConfig(model="llama-3-8b-2l", random_init=True, max_model_len=1024,
                             max_num_seqs=96, max_num_batched_tokens=2048,
                             num_gpu_blocks_override=512, cuda_graph_max_bs=80,
                             quantization="mxfp4"))
g = torch.Generator().manual_seed(1)
seqs = [eng.add_request(torch.randint(100, 128000, (1 + n % 7,), generator=g).tolist(),
                        SamplingParams(temperature=1.0, seed=n, max_tokens=4, ignore_eos=True))
        for n in range(80)]
while eng.has_unfinished():
    eng.step()
ops.debug_check()
assert all(len(s.output_token_ids) == 4 for s in seqs)
assert eng.executor.runner.stats["graph_steps"] > 0
c = gemm.w4_counts()
assert c["k9mf"] > 0 and c["k9mf_silu"] > 0, c
assert any(k[0] > 64 for k in gemm.w4_dg_plan())
print("W4-MID-DEBUG-BUILD-OK", c)
'''


def test_quantized_mid_bucket_engine_in_the_debug_build(gpu):
    """The quantised engine with a decode bucket above 64 (K9mf, force mode) on the
    bounds-checking library, in a child process: one process cannot load both builds."""
    so = os.path.join(ROOT, "kubernetes_gpu_cluster_amd", "_kgc_ops_debug.so")
    if not os.path.exists(so):
        pytest.fail("debug build missing: run KGC_HIP_DEBUG=1 python csrc/build.py")
    pp = os.environ.get("PYTHONPATH", "")
    env = dict(os.environ, KGC_HIP_DEBUG="1", KGC_W4_DGEMM="force",
               PYTHONPATH=os.pathsep.join([p for p in pp.split(os.pathsep) if p] + [ROOT]))
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "W4-MID-DEBUG-BUILD-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
