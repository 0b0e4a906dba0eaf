"""Numerics of every gfx950 HIP kernel vs the fp32 PyTorch reference (ops.reference)."""
import math
import os

import pytest
import torch

import sampler_oracle as so
from kubernetes_gpu_cluster_amd import ops
from kubernetes_gpu_cluster_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

DT = [torch.bfloat16, torch.float16]


def _tol(dt):
    return dict(atol=2e-2, rtol=2e-2) if dt == torch.bfloat16 else dict(atol=5e-3, rtol=5e-3)


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("H", [256, 4096, 5120, 8192])
def test_rms_norm(gpu, dt, H):
    torch.manual_seed(0)
    x = torch.randn(37, H, dtype=dt, device=gpu)
    w = torch.randn(H, dtype=dt, device=gpu)
    out = ops.rms_norm(x, w, 1e-5)
    torch.testing.assert_close(out.float(), ref.rms_norm(x.cpu(), w.cpu(), 1e-5).float().to(gpu),
                               **_tol(dt))


@pytest.mark.parametrize("dt", DT)
def test_fused_add_rms_norm(gpu, dt):
    torch.manual_seed(1)
    x = torch.randn(64, 4096, dtype=dt, device=gpu)
    r = torch.randn(64, 4096, dtype=dt, device=gpu)
    w = torch.randn(4096, dtype=dt, device=gpu)
    eo, er = ref.fused_add_rms_norm(x.cpu(), r.cpu(), w.cpu(), 1e-6)
    x2, r2 = ops.fused_add_rms_norm(x.clone(), r.clone(), w, 1e-6)
    torch.testing.assert_close(r2.cpu().float(), er.float(), atol=0, rtol=0)
    torch.testing.assert_close(x2.cpu().float(), eo.float(), **_tol(dt))


def test_layer_norm(gpu):
    x = torch.randn(9, 768, dtype=torch.float16, device=gpu)
    w, b = torch.randn(768, dtype=torch.float16, device=gpu), torch.randn(768, dtype=torch.float16, device=gpu)
    torch.testing.assert_close(ops.layer_norm(x, w, b).float().cpu(),
                               ref.layer_norm(x.cpu(), w.cpu(), b.cpu()).float(), atol=1e-2, rtol=1e-2)


@pytest.mark.parametrize("dt", DT)
def test_silu_mul(gpu, dt):
    x = torch.randn(100, 2 * 14336, dtype=dt, device=gpu)
    torch.testing.assert_close(ops.silu_mul(x).float().cpu(), ref.silu_mul(x.cpu()).float(), **_tol(dt))


def _cache(nb, nkv, bs, d, dt, dev):
    kc = torch.zeros(nb, nkv, bs, d, dtype=dt, device=dev)
    vc = torch.zeros(nb, nkv, bs // 8, d, 8, dtype=dt, device=dev)
    return kc, vc


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("qk_norm", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_rope_kv_write(gpu, dt, qk_norm, d):
    torch.manual_seed(2)
    T, nq, nkv, bs, nb = 50, 8, 2, 16, 20
    qkv = torch.randn(T, (nq + 2 * nkv) * d, dtype=dt, device=gpu)
    pos = torch.randint(0, 1000, (T,), device=gpu)
    slots = torch.randperm(nb * bs, device=gpu)[:T]
    slots[3] = -1
    cs = ref.rope_cos_sin_cache(d, 2048, 5e5).to(gpu)
    qn = torch.randn(d, dtype=dt, device=gpu) if qk_norm else None
    kn = torch.randn(d, dtype=dt, device=gpu) if qk_norm else None
    kc, vc = _cache(nb, nkv, bs, d, dt, gpu)
    kc2, vc2 = kc.cpu().clone(), vc.cpu().clone()
    q = ops.rope_kv_write(qkv, pos, cs, kc, vc, slots, nq, nkv, d, qn, kn, 1e-6)
    qr = ref.rope_qk_kv_write(qkv.cpu(), pos.cpu(), cs.cpu(), kc2, vc2, slots.cpu(), nq, nkv, d,
                              None if qn is None else qn.cpu(), None if kn is None else kn.cpu(), 1e-6)
    torch.testing.assert_close(q.cpu().float(), qr.float(), **_tol(dt))
    torch.testing.assert_close(kc.cpu().float(), kc2.float(), **_tol(dt))
    torch.testing.assert_close(vc.cpu().float(), vc2.float(), atol=0, rtol=0)


@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("qk_norm", [False, True])
def test_rope_kv_write_from_splitk_slices(gpu, S, qk_norm):
    """The K9m QKV slices (fp32 [S, T, N]) summed inside rope_kv_write == rope_kv_write on
    the bf16-rounded sum (what a separate reduction kernel would hand it), bit for bit."""
    torch.manual_seed(7 + S)
    T, nq, nkv, d, bs, nb = 40, 8, 2, 128, 16, 12
    N = (nq + 2 * nkv) * d
    sl = torch.randn(S, T, N, dtype=torch.float32, device=gpu)
    pos = torch.randint(0, 1000, (T,), device=gpu)
    slots = torch.randperm(nb * bs, device=gpu)[:T]
    cs = ref.rope_cos_sin_cache(d, 2048, 5e5).to(gpu)
    qn = torch.randn(d, dtype=torch.bfloat16, device=gpu) if qk_norm else None
    kn = torch.randn(d, dtype=torch.bfloat16, device=gpu) if qk_norm else None
    kc, vc = _cache(nb, nkv, bs, d, torch.bfloat16, gpu)
    kc2, vc2 = kc.clone(), vc.clone()
    q = ops.rope_kv_write(sl, pos, cs, kc, vc, slots, nq, nkv, d, qn, kn, 1e-6,
                          dtype=torch.bfloat16)
    summed = sl[0].clone()
    for z in range(1, S):
        summed += sl[z]
    q2 = ops.rope_kv_write(summed.to(torch.bfloat16), pos, cs, kc2, vc2, slots, nq, nkv, d, qn,
                           kn, 1e-6)
    assert q.dtype == torch.bfloat16
    torch.testing.assert_close(q, q2, atol=0, rtol=0)
    torch.testing.assert_close(kc, kc2, atol=0, rtol=0)
    torch.testing.assert_close(vc, vc2, atol=0, rtol=0)


def _fill_random_cache(B, ctx_lens, nkv, bs, d, dt, dev, nb_extra=7):
    max_blocks = max(math.ceil(c / bs) for c in ctx_lens) + 1
    nb = sum(math.ceil(c / bs) for c in ctx_lens) + nb_extra
    kc = (torch.randn(nb, nkv, bs, d, device=dev) * 0.5).to(dt)
    vc = torch.randn(nb, nkv, bs // 8, d, 8, device=dev).to(dt)
    perm = torch.randperm(nb).tolist()
    bt = torch.zeros(B, max_blocks, dtype=torch.int32)
    k = 0
    for b, c in enumerate(ctx_lens):
        n = math.ceil(c / bs)
        bt[b, :n] = torch.tensor(perm[k:k + n])
        k += n
    return kc, vc, bt.to(dev)


# decode kernel per launch: K1w (one wave per z-slice) from DECODE_WAVE_MIN_PAIRS (seq, kv-head)
# pairs up -- with slices of at least 2 chunks, or ("wave1") a minimum so large that every
# context is ONE slice writing its output directly (the many-pairs form) -- and the 4-wave
# kernel below; the overrides run all three on every shape
_DECODE_KERNELS = {"wave": ("1", "2"), "wave1": ("1", "100000"), "four": ("1000000000", "2")}


def _use_decode_kernel(monkeypatch, kern):
    pairs, min_chunks = _DECODE_KERNELS[kern]
    monkeypatch.setenv("KGC_DECODE_WAVE_MIN_PAIRS", pairs)
    monkeypatch.setenv("KGC_DECODE_MIN_CHUNKS", min_chunks)


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("d,nq,nkv", [(128, 32, 8), (128, 8, 1), (128, 28, 4), (64, 12, 12),
                                      (128, 16, 16)])
@pytest.mark.parametrize("bs", [16, 32])
@pytest.mark.parametrize("kern", list(_DECODE_KERNELS))
def test_paged_decode(gpu, monkeypatch, kern, dt, d, nq, nkv, bs):
    """K1 vs the fp32 reference at ragged lengths (1 token .. 2049), GQA 1/4/7/8 and MHA,
    z = 1, 3 and 40 (K1w: most slices of the short rows empty, the reduce merges only the
    used ones)."""
    _use_decode_kernel(monkeypatch, kern)
    torch.manual_seed(3)
    ctx = [1, 17, 128, 129, 300, 1000, 2049, 64]
    B = len(ctx)
    kc, vc, bt = _fill_random_cache(B, ctx, nkv, bs, d, dt, gpu)
    q = torch.randn(B, nq, d, dtype=dt, device=gpu)
    cl = torch.tensor(ctx, dtype=torch.int32, device=gpu)
    scale = d ** -0.5
    for z in (1, 3, 40):
        out = ops.paged_attention_decode(q, kc, vc, bt, cl, scale, grid_z=z)
        exp = ref.paged_attention_decode(q.cpu(), kc.cpu(), vc.cpu(), bt.cpu(), cl.cpu(), scale)
        torch.testing.assert_close(out.cpu().float(), exp.float(), **_tol(dt))


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("d,nq,nkv", [(128, 32, 8), (64, 8, 2), (128, 16, 16), (128, 8, 1), (64, 2, 1)])
@pytest.mark.parametrize("qk_norm", [False, True])
@pytest.mark.parametrize("S", [0, 3, 5])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("kern", list(_DECODE_KERNELS))
def test_paged_decode_rope(gpu, monkeypatch, kern, dt, d, nq, nkv, qk_norm, S, fp8):
    """The decode kernel with rope_kv_write folded in == rope_kv_write + paged_decode on
    the same inputs (q / k / v and the cache update), and == the fp32 reference.  One row
    is graph padding (ctx 0, slot -1): nothing of it reaches the cache."""
    _use_decode_kernel(monkeypatch, kern)
    torch.manual_seed(17 + d + S)
    bs = 16
    ctx = [1, 17, 300, 1000, 0, 64, 129]
    B = len(ctx)
    kc, vc, bt = _fill_random_cache(B, [max(c, 1) for c in ctx], nkv, bs, d, dt, gpu)
    ks = vs = 1.0
    if fp8:
        ks, vs = 0.05, 0.07
        kc = (kc.float() / ks).to(torch.float8_e4m3fn)
        vc = (vc.float() / vs).to(torch.float8_e4m3fn)
    N = (nq + 2 * nkv) * d
    if S:
        qkv = torch.randn(S, B, N, dtype=torch.float32, device=gpu)
        summed = qkv[0].clone()           # summed in the kernel's order (z = 0, 1, ...)
        for z in range(1, S):
            summed += qkv[z]
        summed = summed.to(dt)
    else:
        qkv = torch.randn(B, N, dtype=dt, device=gpu)
        summed = qkv
    pos = torch.tensor([max(c - 1, 0) for c in ctx], device=gpu)
    slots = torch.tensor([int(bt[b, (c - 1) // bs]) * bs + (c - 1) % bs if c else -1
                          for b, c in enumerate(ctx)], device=gpu)
    cs = ref.rope_cos_sin_cache(d, 4096, 5e5).to(gpu)
    qn = torch.randn(d, dtype=dt, device=gpu) if qk_norm else None
    kn = torch.randn(d, dtype=dt, device=gpu) if qk_norm else None
    cl = torch.tensor(ctx, dtype=torch.int32, device=gpu)
    scale = d ** -0.5
    tol = _tol(dt) if not fp8 else dict(atol=6e-2, rtol=6e-2)
    kc0, vc0 = kc.clone(), vc.clone()
    for z in (1, 3):
        kc1, vc1 = kc0.clone(), vc0.clone()
        out = ops.paged_attention_decode_rope(qkv, pos, cs, kc1, vc1, slots, nq, nkv, d, bt, cl,
                                              scale, qn, kn, 1e-6, grid_z=z, k_scale=ks,
                                              v_scale=vs, dtype=dt)
        kc2, vc2 = kc0.clone(), vc0.clone()
        q2 = ops.rope_kv_write(summed, pos, cs, kc2, vc2, slots, nq, nkv, d, qn, kn, 1e-6,
                               k_scale=ks, v_scale=vs)
        out2 = ops.paged_attention_decode(q2, kc2, vc2, bt, cl, scale, grid_z=z, k_scale=ks,
                                          v_scale=vs)
        # v is moved, not computed: bit for bit.  k / q may differ in the last bit (the
        # q/k-norm sum order, FMA contraction of the rotation).
        torch.testing.assert_close(vc1.view(torch.uint8), vc2.view(torch.uint8), atol=0, rtol=0)
        # fp8: a last-bit difference before quantisation can move a value across an e4m3
        # rounding boundary: one e4m3 step (2^-3 relative) on the rare element
        torch.testing.assert_close(kc1.float(), kc2.float(),
                                   **(dict(atol=1e-3, rtol=0.13) if fp8 else tol))
        torch.testing.assert_close(out.float(), out2.float(), **tol)
        # fp32 reference of the whole fused op (CPU)
        kc3, vc3 = kc0.cpu().clone(), vc0.cpu().clone()
        qr = ref.rope_qk_kv_write(summed.cpu(), pos.cpu(), cs.cpu(), kc3, vc3, slots.cpu(), nq,
                                  nkv, d, None if qn is None else qn.cpu(),
                                  None if kn is None else kn.cpu(), 1e-6, True, ks, vs)
        exp = ref.paged_attention_decode(qr, kc3, vc3, bt.cpu(), cl.cpu(), scale, ks, vs)
        torch.testing.assert_close(out.cpu().float(), exp.float(), **tol)


def test_paged_decode_single_slice_rows_many_pairs(gpu, monkeypatch):
    """at >= DECODE_LONG_PAIRS (seq, kv-head) pairs K1w keeps contexts of up to
    10 chunks in ONE slice, written directly (nused == 1), while longer contexts in the same
    launch write partials for the merge -- both kernels must derive the same plan from the
    one min_per value.  B = 256, nq 8 / nkv 1 (the 70B TP = 8 rank's heads), contexts of 0
    (graph idle rows), 1 .. 320 (one slice) and 321 .. 1500 (several), at the engine's grid
    and at a forced deep grid; the idle rows must come out zero."""
    for v in ("KGC_DECODE_WAVE_MIN_PAIRS", "KGC_DECODE_MIN_CHUNKS"):
        monkeypatch.delenv(v, raising=False)
    torch.manual_seed(21)
    B, nq, nkv, d, bs = 256, 8, 1, 128, 32
    g = torch.Generator().manual_seed(5)
    ctx = torch.randint(1, 1500, (B,), generator=g)
    ctx[::7] = torch.randint(1, 320, (len(ctx[::7]),), generator=g)
    ctx[3::11] = 0
    ctx[5] = 320
    ctx[6] = 321
    kc, vc, bt = _fill_random_cache(B, [max(int(c), 1) for c in ctx], nkv, bs, d,
                                    torch.bfloat16, gpu)
    q = torch.randn(B, nq, d, dtype=torch.bfloat16, device=gpu)
    cl = ctx.to(torch.int32).to(gpu)
    exp = ref.paged_attention_decode(q.cpu(), kc.cpu(), vc.cpu(), bt.cpu(), cl.cpu(), d ** -0.5)
    assert ops.decode_uses_wave(B, nkv)
    for z in (ops.decode_grid_z(B, nkv, 4096), 16):
        out = torch.full_like(q, float("nan"))
        out = ops.paged_attention_decode(q, kc, vc, bt, cl, d ** -0.5, grid_z=z, out=out)
        torch.testing.assert_close(out.cpu().float(), exp.float(), **_tol(torch.bfloat16))
        assert torch.all(out[ctx.to(gpu) == 0] == 0)


@pytest.mark.parametrize("kern", list(_DECODE_KERNELS))
def test_paged_decode_workspace_reuse(gpu, monkeypatch, kern):
    """One static partials workspace serves launches of any Z (incl. an empty context),
    eager or replayed from a graph."""
    _use_decode_kernel(monkeypatch, kern)
    torch.manual_seed(13)
    dt, d, nq, nkv, bs = torch.bfloat16, 128, 32, 8, 32
    ctx = [1, 700, 2049, 64, 0, 333]
    B = len(ctx)
    kc, vc, bt = _fill_random_cache(B, [max(c, 1) for c in ctx], nkv, bs, d, dt, gpu)
    q = torch.randn(B, nq, d, dtype=dt, device=gpu)
    cl = torch.tensor(ctx, dtype=torch.int32, device=gpu)
    ws = ops.decode_partials(B, nq, d, bt.shape[1], bs, gpu)
    exp = ref.paged_attention_decode(q.cpu(), kc.cpu(), vc.cpu(), bt.cpu(), cl.cpu(), d ** -0.5)
    for z in (7, 1, 16, 3, 16):
        out = ops.paged_attention_decode(q, kc, vc, bt, cl, d ** -0.5, workspace=ws, grid_z=z)
        torch.testing.assert_close(out.cpu().float(), exp.float(), **_tol(dt))
    out = torch.empty_like(q)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.paged_attention_decode(q, kc, vc, bt, cl, d ** -0.5, workspace=ws, grid_z=5, out=out)
    for _ in range(3):
        out.zero_()
        g.replay()
        torch.testing.assert_close(out.cpu().float(), exp.float(), **_tol(dt))


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("d,nq,nkv", [(128, 32, 8), (64, 4, 4), (128, 8, 1), (64, 2, 1)])
def test_prefill_attention(gpu, dt, d, nq, nkv):
    torch.manual_seed(4)
    bs = 16
    seq_lens = [5, 130, 300, 64, 700]
    query_lens = [5, 130, 100, 1, 257]      # 3 chunked-prefill continuations
    kc, vc, bt = _fill_random_cache(len(seq_lens), seq_lens, nkv, bs, d, dt, gpu)
    qsl = [0]
    for ql in query_lens:
        qsl.append(qsl[-1] + ql)
    q = torch.randn(qsl[-1], nq, d, dtype=dt, device=gpu)
    qsl_t = torch.tensor(qsl, dtype=torch.int32, device=gpu)
    sl_t = torch.tensor(seq_lens, dtype=torch.int32, device=gpu)
    out = ops.prefill_attention(q, kc, vc, bt, qsl_t, sl_t, d ** -0.5)
    exp = ref.prefill_attention(q.cpu(), kc.cpu(), vc.cpu(), bt.cpu(), qsl_t.cpu(), sl_t.cpu(),
                                d ** -0.5)
    torch.testing.assert_close(out.cpu().float(), exp.float(), **_tol(dt))


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("gqa,d,nq,nkv", [("1", 128, 32, 8), ("0", 128, 32, 8),
                                         ("1", 128, 64, 8), ("0", 64, 4, 4),
                                         ("1", 64, 2, 1), ("1", 128, 8, 1)])
@pytest.mark.parametrize("kvg", ["1", "0"])
def test_prefill_rope_fused_equals_unfused(gpu, monkeypatch, dt, gqa, d, nq, nkv, kvg):
    """Prefill-only step with q RoPE folded into K2's q load (kv_write_rope +
    prefill_attention_rope) vs rope_kv_write + prefill_attention: the same K/V cache bytes,
    the same attention output (the rotation is one shared helper, rounded the same way),
    and both within tolerance of the fp32 reference.  Fresh prompts and chunked
    continuations (positions = context start + row), GQA-shared and one-head kernels."""
    monkeypatch.setenv("KGC_PREFILL_GQA", gqa)
    monkeypatch.setenv("KGC_ROPE_KVG", kvg)           # 8-token-group K / V kernel on / off
    torch.manual_seed(11)
    bs = 16
    seq_lens = [5, 130, 300, 64, 700]
    query_lens = [5, 130, 100, 1, 257]
    kc, vc, bt = _fill_random_cache(len(seq_lens), seq_lens, nkv, bs, d, dt, gpu)
    qsl = [0]
    for ql in query_lens:
        qsl.append(qsl[-1] + ql)
    T = qsl[-1]
    N = (nq + 2 * nkv) * d
    qkv = torch.randn(T, N + 64, dtype=dt, device=gpu)[:, :N]     # padded row stride
    pos, slots = [], []
    btc = bt.cpu()
    for i, (L, ql) in enumerate(zip(seq_lens, query_lens)):
        for p in range(L - ql, L):
            pos.append(p)
            slots.append(int(btc[i, p // bs]) * bs + p % bs)
    pos_t = torch.tensor(pos, dtype=torch.int64, device=gpu)
    slot_t = torch.tensor(slots, dtype=torch.int64, device=gpu)
    cs = ref.rope_cos_sin_cache(d, 1024, 500000.0).to(gpu)
    qsl_t = torch.tensor(qsl, dtype=torch.int32, device=gpu)
    sl_t = torch.tensor(seq_lens, dtype=torch.int32, device=gpu)
    kc1, vc1, kc2, vc2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    q = ops.rope_kv_write(qkv, pos_t, cs, kc1, vc1, slot_t, nq, nkv, d)
    out1 = ops.prefill_attention(q, kc1, vc1, bt, qsl_t, sl_t, d ** -0.5)
    ops.kv_write_rope(qkv, pos_t, cs, kc2, vc2, slot_t, nq, nkv, d)
    out2 = ops.prefill_attention_rope(qkv, cs, kc2, vc2, bt, qsl_t, sl_t, d ** -0.5, nq, d)
    torch.cuda.synchronize()
    assert torch.equal(kc1, kc2) and torch.equal(vc1, vc2)
    torch.testing.assert_close(out2.cpu().float(), out1.cpu().float(), atol=1e-6, rtol=0)
    kr, vr = kc.cpu().clone(), vc.cpu().clone()
    qr = ref.rope_qk_kv_write(qkv.cpu().contiguous(), pos_t.cpu(), cs.cpu(), kr, vr, slot_t.cpu(), nq, nkv, d,
                              None, None, 1e-6, True, 1.0, 1.0)
    exp = ref.prefill_attention(qr, kr, vr, bt.cpu(), qsl_t.cpu(), sl_t.cpu(), d ** -0.5)
    torch.testing.assert_close(out2.cpu().float(), exp.float(), **_tol(dt))
    # V is a pure copy: the coalesced whole-group V^T stores and the per-token scatter
    # (partial groups, chunk boundaries) must reproduce the reference cache exactly
    assert torch.equal(vc1.cpu(), vr)


@pytest.mark.parametrize("gqa,nq,nkv,S", [("1", 32, 8, 8192), ("0", 32, 8, 8192),
                                         ("1", 32, 8, 2048), ("1", 64, 8, 2048),
                                         ("1", 16, 2, 2048), ("0", 64, 8, 2048)])
def test_prefill_long_gqa_matches_fp32(gpu, monkeypatch, gqa, nq, nkv, S):
    """K2 at long prompts (2K / 8K tokens: a fresh prompt plus a chunked continuation),
    GQA groups of 4 and 8 through the GQA-shared kernel (KGC_PREFILL_GQA=1, one workgroup
    per kv head x query block) and through the one-head kernel (=0), vs an fp32 dense
    causal reference."""
    monkeypatch.setenv("KGC_PREFILL_GQA", gqa)
    torch.manual_seed(S + nq)
    d, bs, dt = 128, 32, torch.bfloat16
    seq_lens, query_lens = [S, S // 2 + 77], [S, 333]
    kc, vc, bt = _fill_random_cache(len(seq_lens), seq_lens, nkv, bs, d, dt, gpu)
    qsl = [0]
    for ql in query_lens:
        qsl.append(qsl[-1] + ql)
    q = torch.randn(qsl[-1], nq, d, dtype=dt, device=gpu)
    qsl_t = torch.tensor(qsl, dtype=torch.int32, device=gpu)
    sl_t = torch.tensor(seq_lens, dtype=torch.int32, device=gpu)
    out = ops.prefill_attention(q, kc, vc, bt, qsl_t, sl_t, d ** -0.5).cpu().float()
    for i in range(2):
        L, ql = seq_lens[i], query_lens[i]
        nbk = (L + bs - 1) // bs
        blocks = bt[i, :nbk].cpu().long()
        k = kc.cpu()[blocks].permute(0, 2, 1, 3).reshape(nbk * bs, nkv, d)[:L].float()
        v = vc.cpu()[blocks].permute(0, 2, 4, 1, 3).reshape(nbk * bs, nkv, d)[:L].float()
        # a sample of query rows (all of the first and last 64, 128 in between), each
        # against all its causal keys: dense fp32 attention
        rows = torch.cat([torch.arange(min(64, ql)), torch.arange(max(0, ql - 64), ql),
                          torch.randint(0, ql, (128,))]).unique()
        qi = q.cpu()[qsl[i]:qsl[i + 1]][rows].float()
        rep = nq // nkv
        kk = k.repeat_interleave(rep, 1).permute(1, 0, 2)           # [nq, L, d]
        vv = v.repeat_interleave(rep, 1).permute(1, 0, 2)
        sc = torch.einsum("qhd,hkd->hqk", qi, kk) * d ** -0.5
        pos = (L - ql + rows)[:, None]
        sc = sc.masked_fill(torch.arange(L)[None, :] > pos, float("-inf"))
        exp = torch.einsum("hqk,hkd->qhd", torch.softmax(sc, -1), vv)
        torch.testing.assert_close(out[qsl[i]:qsl[i + 1]][rows], exp, atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("gqa", ["1", "0"])
@pytest.mark.parametrize("shape", ["ramp", "steps"])
def test_prefill_lazy_rescale_growing_scores(gpu, monkeypatch, gqa, shape):
    """K2's lazy O rescale (PF_RESCALE_THR) on scores whose row max keeps GROWING along
    the keys -- the branch random data never takes: every row's running max moves by
    small steps (skipped: P up to 2^8 at the stale max) and by jumps (rescale of O, l and
    m together), on the diagonal tiles and off them.  fp32 dense causal reference."""
    monkeypatch.setenv("KGC_PREFILL_GQA", gqa)
    torch.manual_seed(7)
    d, bs, dt, nq, nkv = 128, 32, torch.bfloat16, 32, 8
    seq_lens, query_lens = [2048, 1500], [2048, 300]
    kc, vc, bt = _fill_random_cache(len(seq_lens), seq_lens, nkv, bs, d, dt, gpu)
    kc_cpu = kc.cpu().float()
    for i, L in enumerate(seq_lens):
        pos = torch.arange(L).float()
        if shape == "ramp":        # ~2 log2 units per 64-key tile: rescale every few tiles
            a = pos * (120.0 / 2048)
        else:                      # flat stretches and jumps of ~12 log2 units
            a = torch.floor(pos / 300) * 25.0
        nbk = (L + bs - 1) // bs
        for j in range(nbk):
            b = int(bt[i, j])
            n = min(bs, L - j * bs)
            kc_cpu[b, :, :n, :] += (a[j * bs:j * bs + n] / d)[None, :, None]
    kc = kc_cpu.to(dt).to(gpu)
    qsl = [0]
    for ql in query_lens:
        qsl.append(qsl[-1] + ql)
    q = (torch.randn(qsl[-1], nq, d) * 0.5 + 4.0).to(dt).to(gpu)
    qsl_t = torch.tensor(qsl, dtype=torch.int32, device=gpu)
    sl_t = torch.tensor(seq_lens, dtype=torch.int32, device=gpu)
    out = ops.prefill_attention(q, kc, vc, bt, qsl_t, sl_t, d ** -0.5).cpu().float()
    assert torch.isfinite(out).all()
    for i in range(2):
        L, ql = seq_lens[i], query_lens[i]
        nbk = (L + bs - 1) // bs
        blocks = bt[i, :nbk].cpu().long()
        k = kc.cpu()[blocks].permute(0, 2, 1, 3).reshape(nbk * bs, nkv, d)[:L].float()
        v = vc.cpu()[blocks].permute(0, 2, 4, 1, 3).reshape(nbk * bs, nkv, d)[:L].float()
        rows = torch.cat([torch.arange(min(96, ql)), torch.arange(max(0, ql - 64), ql),
                          torch.randint(0, ql, (128,))]).unique()
        qi = q.cpu()[qsl[i]:qsl[i + 1]][rows].float()
        rep = nq // nkv
        kk = k.repeat_interleave(rep, 1).permute(1, 0, 2)
        vv = v.repeat_interleave(rep, 1).permute(1, 0, 2)
        sc = torch.einsum("qhd,hkd->hqk", qi, kk) * d ** -0.5
        posq = (L - ql + rows)[:, None]
        sc = sc.masked_fill(torch.arange(L)[None, :] > posq, float("-inf"))
        exp = torch.einsum("hqk,hkd->qhd", torch.softmax(sc, -1), vv)
        torch.testing.assert_close(out[qsl[i]:qsl[i + 1]][rows], exp, atol=3e-2, rtol=3e-2)


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("nq,nkv,d", [(32, 8, 128), (64, 8, 128), (8, 1, 128), (16, 4, 64)])
@pytest.mark.parametrize("shape", ["short_many", "mixed_chunked", "one_item"])
def test_prefill_persistent_walk_bit_identical(gpu, monkeypatch, dt, nq, nkv, d, shape):
    """K2's persistent GQA walk (one workgroup per CU over the work list, the K / V tile
    stream running across items; KGC_PREFILL_PERSIST=1, the default) against the one-shot
    GQA grid (=0): the same tiles in the same order per wave, so the outputs must agree bit
    for bit -- on many short prompts (more items than CUs, 1-8 tiles each), on mixed fresh
    prompts and chunked continuations (empty sub-blocks, single-tile items next to long
    ones), and on a single item -- and both within tolerance of the fp32 reference; the
    walk also replays correctly from a captured graph."""
    monkeypatch.setenv("KGC_PREFILL_GQA", "1")
    torch.manual_seed(21)
    bs = 16
    if shape == "short_many":
        seq_lens = [512] * 24 + [96, 33, 64, 1, 200]
        query_lens = list(seq_lens)
    elif shape == "mixed_chunked":
        seq_lens = [5, 130, 300, 64, 700, 1030, 17]
        query_lens = [5, 130, 100, 1, 257, 1030, 3]
    else:
        seq_lens, query_lens = [40], [40]
    kc, vc, bt = _fill_random_cache(len(seq_lens), seq_lens, nkv, bs, d, dt, gpu)
    qsl = [0]
    for ql in query_lens:
        qsl.append(qsl[-1] + ql)
    q = torch.randn(qsl[-1], nq, d, dtype=dt, device=gpu)
    qsl_t = torch.tensor(qsl, dtype=torch.int32, device=gpu)
    sl_t = torch.tensor(seq_lens, dtype=torch.int32, device=gpu)
    outs = {}
    for persist in ("0", "1"):
        monkeypatch.setenv("KGC_PREFILL_PERSIST", persist)
        outs[persist] = ops.prefill_attention(q, kc, vc, bt, qsl_t, sl_t, d ** -0.5)
    torch.cuda.synchronize()
    assert torch.equal(outs["0"], outs["1"])
    if shape != "short_many" or nq == 32:
        exp = ref.prefill_attention(q.cpu(), kc.cpu(), vc.cpu(), bt.cpu(), qsl_t.cpu(),
                                    sl_t.cpu(), d ** -0.5)
        torch.testing.assert_close(outs["1"].cpu().float(), exp.float(), **_tol(dt))
    # graph replay of the persistent walk
    monkeypatch.setenv("KGC_PREFILL_PERSIST", "1")
    ws, wm = ops.prefill_work_list(query_lens, seq_lens)
    ws_t = torch.tensor(ws, dtype=torch.int32, device=gpu)
    wm_t = torch.tensor(wm, dtype=torch.int32, device=gpu)
    out = torch.empty_like(q)
    ops.prefill_attention(q, kc, vc, bt, qsl_t, sl_t, d ** -0.5, ws_t, wm_t, out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.prefill_attention(q, kc, vc, bt, qsl_t, sl_t, d ** -0.5, ws_t, wm_t, out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, outs["0"])


def test_prefill_matches_dense(gpu):
    """End-to-end: rope_kv_write -> prefill kernel == dense causal attention."""
    torch.manual_seed(5)
    S, nq, nkv, d, bs = 333, 8, 2, 128, 32
    dt = torch.bfloat16
    qkv = torch.randn(S, (nq + 2 * nkv) * d, dtype=dt, device=gpu)
    pos = torch.arange(S, device=gpu)
    nb = math.ceil(S / bs)
    kc, vc = _cache(nb + 1, nkv, bs, d, dt, gpu)
    slots = torch.arange(S, device=gpu) + bs  # blocks 1..nb
    bt = torch.arange(1, nb + 1, dtype=torch.int32, device=gpu)[None]
    cs = ref.rope_cos_sin_cache(d, 4096, 1e4).to(gpu)
    q = ops.rope_kv_write(qkv, pos, cs, kc, vc, slots, nq, nkv, d)
    out = ops.prefill_attention(q, kc, vc, bt, torch.tensor([0, S], dtype=torch.int32, device=gpu),
                                torch.tensor([S], dtype=torch.int32, device=gpu), d ** -0.5)
    k = ref.apply_rope(qkv[:, nq * d:(nq + nkv) * d].reshape(S, nkv, d).cpu(), pos.cpu(), cs.cpu())
    v = qkv[:, (nq + nkv) * d:].reshape(S, nkv, d).cpu()
    exp = ref.dense_causal_attention(q.cpu(), k, v, d ** -0.5)
    torch.testing.assert_close(out.cpu().float(), exp.float(), atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("B", [16, 1, 4, 256, 260])
def test_sample(gpu, dt, B):
    """B <= 256: the cooperative kernel (threshold passes split over each row's
    workgroups, per-row barriers); B = 260: the single-workgroup-per-threshold kernel."""
    torch.manual_seed(6)
    V = 128256
    logits = (torch.randn(B, V, device=gpu) * 3).to(dt)
    reps = (B + 3) // 4
    temp = torch.tensor([0.0, 1.0, 0.7, 1.3] * reps, device=gpu)[:B]
    top_k = torch.tensor([-1, -1, 50, -1] * reps, dtype=torch.int32, device=gpu)[:B]
    top_p = torch.tensor([1.0, 1.0, 1.0, 0.9] * reps, device=gpu)[:B]
    seeds = torch.arange(B, dtype=torch.int64, device=gpu) * 7919 + (5 << 32)
    got = ops.sample(logits, temp, top_k, top_p, seeds).cpu()
    exp = ref.sample(logits.cpu(), temp.cpu(), top_k.cpu(), top_p.cpu(), seeds.cpu())
    # greedy / pure-temperature / top-k rows are exact; every top-p row is judged by the
    # float64 oracle: the one right token, unless the nucleus boundary or the two best
    # scores lie within the fp32 band (tests/sampler_oracle.py)
    exact = [i for i in range(B) if i % 4 != 3]
    assert got[exact].tolist() == exp[exact].tolist()
    nucleus = list(range(3, B, 4))
    if nucleus:
        so.check(got[nucleus], so.judge(logits.cpu()[nucleus], temp.cpu()[nucleus],
                                        top_k.cpu()[nucleus], top_p.cpu()[nucleus],
                                        seeds.cpu()[nucleus]), "top-p rows")
    # rows without thresholds: the single-pass path picks the same ids
    plain = [i for i in range(B) if i % 4 in (0, 1)]
    if plain:
        idx = torch.tensor(plain, device=gpu)
        g2 = ops.sample(logits[idx].contiguous(), temp[idx], top_k[idx], top_p[idx], seeds[idx],
                        thresholds=False).cpu()
        assert g2.tolist() == got[plain].tolist()


@pytest.mark.parametrize("B", [2, 8])
def test_sample_threshold_ties_overflow_candidates(gpu, B):
    """Integer-valued logits put ~10K tokens in every distance bin: the crossing bin holds
    more than the candidate list (2048), so the cooperative kernel takes the global radix
    passes; a tied top-k boundary keeps the whole tie group, as the reference does."""
    torch.manual_seed(11)
    V = 128256
    logits = (torch.randn(B, V, device=gpu) * 3).round().to(torch.bfloat16)
    temp = torch.ones(B, device=gpu)
    top_k = torch.tensor([50, -1] * (B // 2), dtype=torch.int32, device=gpu)
    top_p = torch.tensor([1.0, 0.9] * (B // 2), device=gpu)
    seeds = torch.arange(B, dtype=torch.int64, device=gpu) * 31 + (9 << 32)
    got = ops.sample(logits, temp, top_k, top_p, seeds).cpu()
    exp = ref.sample(logits.cpu(), temp.cpu(), top_k.cpu(), top_p.cpu(), seeds.cpu())
    assert got[0::2].tolist() == exp[0::2].tolist()
    # top-p rows: the sampled token lies in the reference nucleus (whole tie groups)
    for b in range(1, B, 2):
        row = logits[b].float().cpu()
        probs = torch.softmax(row, -1)
        sp, _ = torch.sort(probs, descending=True)
        keep = (torch.cumsum(sp, 0) - sp) < 0.9
        assert probs[got[b]] >= sp[keep][-1]


def test_sample_distribution(gpu):
    """Gumbel-max frequencies follow softmax(logits / T)."""
    V, N = 8, 20000
    logits = torch.tensor([[0.0, 1.0, 2.0, -1.0, 0.5, 3.0, -2.0, 1.5]], device=gpu).repeat(N, 1)
    temp = torch.full((N,), 1.0, device=gpu)
    got = ops.sample(logits, temp, torch.full((N,), -1, dtype=torch.int32, device=gpu),
                     torch.ones(N, device=gpu), torch.arange(N, dtype=torch.int64, device=gpu))
    freq = torch.bincount(got.cpu(), minlength=V).float() / N
    exp = torch.softmax(logits[0].cpu(), -1)
    assert (freq - exp).abs().max() < 0.015


@pytest.mark.parametrize("tp", [2, 8])
def test_sample_vocab_parallel_equals_unsharded(gpu, tp):
    """K10 vocab-parallel: per-shard packed candidates (global-column noise) + MAX over
    the shards + unpack == the unsharded sampler, bit for bit (greedy and temperature
    rows; padded shard columns excluded); and == the CPU reference."""
    torch.manual_seed(7)
    B, V = 64, 128256
    per = (V + 64 * tp - 1) // (64 * tp) * 64            # ParallelLMHead padding
    logits = (torch.randn(B, per * tp, device=gpu) * 3).to(torch.bfloat16)
    logits[5, 1000] = logits[5, V - 3] = 40.0             # greedy tie across shards
    temp = torch.tensor([0.0, 1.0, 0.7, 1.3] * (B // 4), device=gpu)
    seeds = torch.arange(B, dtype=torch.int64, device=gpu) * 104729 + (3 << 32)
    ones = torch.ones(B, device=gpu)
    full = ops.sample(logits[:, :V].contiguous(), temp, torch.full((B,), -1, dtype=torch.int32,
                      device=gpu), ones, seeds).cpu()
    parts = []
    for r in range(tp):
        shard = logits[:, r * per:(r + 1) * per].contiguous()
        cols = max(0, min(per, V - r * per))
        parts.append(ops.sample_vp_partial(shard, cols, temp, seeds, r * per))
    packed = torch.stack(parts).max(0).values
    got = ops.sample_vp_finish(packed).cpu()
    assert got.tolist() == full.tolist()
    assert got[5].item() == 1000
    # CPU reference of one shard's candidate (index; the fp32 value may differ in ulps)
    r0 = ref.sample_vp_partial(logits[:8, :per].cpu(), temp[:8].cpu(), seeds[:8].cpu(), 0)
    assert ref.sample_vp_unpack(r0).tolist() == ops.sample_vp_finish(parts[0][:8]).cpu().tolist()


# ------------------------------------------------------------------ MoE (K13 / K14)
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("E,k", [(8, 2), (4, 2), (64, 6)])
def test_moe_route(gpu, dt, E, k):
    torch.manual_seed(5)
    logits = torch.randn(300, E, dtype=dt, device=gpu)
    w, ids = ops.moe_topk_softmax(logits, k)
    rw, rids = ref.moe_topk_softmax(logits.cpu(), k)
    # bf16/fp16 logits tie often; torch.topk breaks ties arbitrarily, the kernel by
    # lowest expert id -- so compare the selected logits, and ids where untied
    lc = logits.cpu().float()
    ids = ids.cpu().long()
    torch.testing.assert_close(lc.gather(1, ids), lc.gather(1, rids.long()), atol=0, rtol=0)
    assert len(set(ids[0].tolist())) == k
    untied = (lc.gather(1, rids.long())[:, :, None] == lc[:, None, :]).sum(-1).eq(1).all(1)
    assert torch.equal(ids[untied], rids.long()[untied])
    torch.testing.assert_close(w.cpu(), rw, atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("E,k,H", [(8, 2, 4096), (8, 2, 512), (4, 1, 1024), (16, 4, 2048),
                                   (6, 2, 512)])
@pytest.mark.parametrize("T", [1, 7, 256, 300])
def test_moe_gate_topk_matches_gemm_then_route(gpu, dt, E, k, H, T):
    """The router GEMM fused into the top-k kernel (ops.moe_gate_topk) == the GEMM (logits
    rounded to the activation dtype) followed by the fp32 softmax / top-k reference: the
    same experts where the top-k logits are untied, weights within fp32 rounding."""
    torch.manual_seed(E * 100 + T + H)
    x = (torch.randn(T, H, device=gpu) * 0.5).to(dt)
    wg = (torch.randn(E, H, device=gpu) / H ** 0.5).to(dt)
    got = ops.moe_gate_topk(x, wg, k)
    assert got is not None
    w, ids = got
    logits = (x.float().cpu() @ wg.float().cpu().t()).to(dt).float()
    rw, rids = ref.moe_topk_softmax(logits, k)
    ids = ids.cpu().long()
    # the fused dot products sum in another order than the fp32 reference: compare the
    # selected logits (a near-tie may pick either expert), ids where clearly separated
    torch.testing.assert_close(logits.gather(1, ids), logits.gather(1, rids.long()),
                               atol=2e-2, rtol=2e-2)
    srt = logits.sort(1, descending=True).values
    clear = (srt[:, k - 1] - srt[:, k]).abs() > 5e-2
    assert torch.equal(ids[clear].sort(1).values, rids.long()[clear].sort(1).values)
    torch.testing.assert_close(w.cpu()[clear], rw[clear], atol=2e-2, rtol=2e-2)


def _moe_case(dt, T, E, k, H, I, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(T, H, generator=g) * 0.5).to(dt).to(dev)
    w13 = (torch.randn(E, 2 * I, H, generator=g) / H ** 0.5).to(dt).to(dev)
    w2 = (torch.randn(E, H, I, generator=g) / I ** 0.5).to(dt).to(dev)
    logits = torch.randn(T, E, generator=g).to(dev)
    tw, tid = ref.moe_topk_softmax(logits.cpu(), k)
    return x, w13, w2, tw.to(dev), tid.to(dev)


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("T", [1, 7, 256, 1000])
def test_fused_moe(gpu, dt, T):
    x, w13, w2, tw, tid = _moe_case(dt, T, 8, 2, 512, 384, gpu)
    out = ops.fused_moe(x, w13, w2, tw, tid)
    exp = ref.moe_mlp_local(x.cpu(), w13.cpu(), w2.cpu(), tw.cpu(), tid.cpu())
    torch.testing.assert_close(out.cpu().float(), exp.float(), **_tol(dt))


def test_fused_moe_expert_subset(gpu):
    """Expert-parallel shard: only experts 4..7 live here; other pairs contribute 0."""
    x, w13, w2, tw, tid = _moe_case(torch.bfloat16, 133, 8, 2, 256, 256, gpu, seed=3)
    out = ops.fused_moe(x, w13[4:].contiguous(), w2[4:].contiguous(), tw, tid, expert_offset=4,
                        all_local=False)
    exp = ref.moe_mlp_local(x.cpu(), w13[4:].cpu(), w2[4:].cpu(), tw.cpu(), tid.cpu(), 4)
    torch.testing.assert_close(out.cpu().float(), exp.float(), **_tol(torch.bfloat16))


@pytest.mark.parametrize("T,lo", [(1, 0), (257, 0), (2048, 0), (300, 4), (1, 4)])
def test_grouped_expert_mlp_row_map_combine(gpu, T, lo):
    """The prefill-size MoE path (models/moe.grouped_expert_mlp: one GEMM pair per expert
    over the expert-sorted rows, the weighted combine reading them through the inverse
    permutation, pairs of non-local experts mapped to -1) == the fp32 reference."""
    from kubernetes_gpu_cluster_amd.models.moe import grouped_expert_mlp
    x, w13, w2, tw, tid = _moe_case(torch.bfloat16, T, 8, 2, 512, 384, gpu, seed=T + lo)
    out = grouped_expert_mlp(x, w13[lo:].contiguous(), w2[lo:].contiguous(), tw, tid, lo)
    exp = ref.moe_mlp_local(x.cpu(), w13[lo:].cpu(), w2[lo:].cpu(), tw.cpu(), tid.cpu(), lo)
    torch.testing.assert_close(out.cpu().float(), exp.float(), **_tol(torch.bfloat16))


def test_moe_combine_row_map_bounds(gpu):
    """moe_combine's row map: -1 and indices past y's rows contribute nothing."""
    T, k, H = 4, 2, 256
    y = torch.randn(3, H, device=gpu).to(torch.bfloat16)
    w = torch.rand(T, k, device=gpu)
    rm = torch.tensor([0, -1, 2, 1, 7, -1, 1, 3], dtype=torch.int32, device=gpu)
    out = torch.empty(T, H, dtype=torch.bfloat16, device=gpu)
    torch.ops.kgc.moe_combine(out, y, w, rm)
    yf, wc, rc = y.float().cpu(), w.cpu(), rm.cpu().view(T, k)
    exp = torch.zeros(T, H)
    for t in range(T):
        for j in range(k):
            r = int(rc[t, j])
            if 0 <= r < 3:
                exp[t] += wc[t, j] * yf[r]
    torch.testing.assert_close(out.float().cpu(), exp, atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("S", [1, 3, 8])
@pytest.mark.parametrize("T,all_local", [(5, True), (300, True), (40, False)])
def test_fused_moe_splitk(gpu, monkeypatch, S, T, all_local):
    """Down projection split over S K-slices (fp32 slices summed in moe_combine); S = 3
    leaves uneven slices of the 16 K-tiles."""
    monkeypatch.setenv("KGC_MOE_SPLITK", str(S))
    x, w13, w2, tw, tid = _moe_case(torch.bfloat16, T, 8, 2, 256, 1024, gpu, seed=5)
    lo = 0 if all_local else 2
    out = ops.fused_moe(x, w13[lo:].contiguous(), w2[lo:].contiguous(), tw, tid,
                        expert_offset=lo, all_local=all_local)
    exp = ref.moe_mlp_local(x.cpu(), w13[lo:].cpu(), w2[lo:].cpu(), tw.cpu(), tid.cpu(), lo)
    torch.testing.assert_close(out.cpu().float(), exp.float(), **_tol(torch.bfloat16))


@pytest.mark.parametrize("T", [1, 5, 64, 256, 300])
@pytest.mark.parametrize("bm", [64, 96, 128])
@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("bn", ["128", "256"])
def test_fused_moe_packed_k14m(gpu, monkeypatch, T, bm, S, bn):
    """K14m (moe_dgemm: the grouped gate_up with its SiLU epilogue and the grouped down
    with its row scatter, on the K9m LDS-DMA pipeline over per-expert packed tiles) vs the
    fp32 reference: row blocks of 64 / 128 (padding rows gathered but never stored), the
    down projection's fp32 K-slices summed in moe_combine, and an expert-parallel shard
    (experts 2..7 here; pairs of the others add 0)."""
    monkeypatch.setenv("KGC_MOE_BM", str(bm))
    monkeypatch.setenv("KGC_MOE_BN", bn)
    monkeypatch.setenv("KGC_MOE_SPLITK", str(S))
    x, w13, w2, tw, tid = _moe_case(torch.bfloat16, T, 8, 2, 512, 1024, gpu, seed=11 + T)
    w13p, w2p = ops.moe_pack(w13, True), ops.moe_pack(w2, False)
    out = ops.fused_moe(x, w13, w2, tw, tid, w13p=w13p, w2p=w2p)
    exp = ref.moe_mlp_local(x.cpu(), w13.cpu(), w2.cpu(), tw.cpu(), tid.cpu())
    torch.testing.assert_close(out.cpu().float(), exp.float(), **_tol(torch.bfloat16))
    # the same kernels' result equals the register-staged grouped GEMM's within rounding
    monkeypatch.setenv("KGC_MOE_BM", str(min(bm, 64) if bm != 128 else 128))
    base = ops.fused_moe(x, w13, w2, tw, tid)
    monkeypatch.setenv("KGC_MOE_BM", str(bm))
    torch.testing.assert_close(out.float(), base.float(), **_tol(torch.bfloat16))
    lo = 2
    w13s, w2s = w13[lo:].contiguous(), w2[lo:].contiguous()
    out = ops.fused_moe(x, w13s, w2s, tw, tid, expert_offset=lo, all_local=False,
                        w13p=ops.moe_pack(w13s, True), w2p=ops.moe_pack(w2s, False))
    exp = ref.moe_mlp_local(x.cpu(), w13s.cpu(), w2s.cpu(), tw.cpu(), tid.cpu(), lo)
    torch.testing.assert_close(out.cpu().float(), exp.float(), **_tol(torch.bfloat16))


def test_fused_moe_packed_graph_capture(gpu):
    """K14m captures into a hipGraph (row counts stay on the device) and replays with new
    routes: the decode graphs' form of the Mixtral block."""
    x, w13, w2, tw, tid = _moe_case(torch.bfloat16, 64, 8, 2, 256, 256, gpu, seed=4)
    w13p, w2p = ops.moe_pack(w13, True), ops.moe_pack(w2, False)
    ops.fused_moe(x, w13, w2, tw, tid, w13p=w13p, w2p=w2p)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.fused_moe(x, w13, w2, tw, tid, w13p=w13p, w2p=w2p)
    for seed in (7, 8):
        x2, _, _, tw2, tid2 = _moe_case(torch.bfloat16, 64, 8, 2, 256, 256, gpu, seed=seed)
        x.copy_(x2)
        tw.copy_(tw2)
        tid.copy_(tid2)
        g.replay()
        exp = ref.moe_mlp_local(x.cpu(), w13.cpu(), w2.cpu(), tw.cpu(), tid.cpu())
        torch.testing.assert_close(out.cpu().float(), exp.float(), **_tol(torch.bfloat16))


def test_fused_moe_graph_capture(gpu):
    """No host sync inside: the block captures into a hipGraph and replays with new routes."""
    x, w13, w2, tw, tid = _moe_case(torch.bfloat16, 64, 8, 2, 256, 256, gpu, seed=4)
    ops.fused_moe(x, w13, w2, tw, tid)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.fused_moe(x, w13, w2, tw, tid)
    for seed in (7, 8):
        x2, _, _, tw2, tid2 = _moe_case(torch.bfloat16, 64, 8, 2, 256, 256, gpu, seed=seed)
        x.copy_(x2)
        tw.copy_(tw2)
        tid.copy_(tid2)
        g.replay()
        exp = ref.moe_mlp_local(x.cpu(), w13.cpu(), w2.cpu(), tw.cpu(), tid.cpu())
        torch.testing.assert_close(out.cpu().float(), exp.float(), **_tol(torch.bfloat16))


# ------------------------------------------------------------------ fp8 KV cache
FP8 = torch.float8_e4m3fn


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("scales", [(1.0, 1.0), (0.5, 2.0)])
def test_rope_kv_write_fp8(gpu, dt, scales):
    """Quantised cache bytes == torch's RNE fp8 conversion of the T-rounded values."""
    torch.manual_seed(12)
    T, nq, nkv, bs, nb, d = 40, 8, 2, 16, 12, 128
    qkv = (torch.randn(T, (nq + 2 * nkv) * d) * 4).to(dt).to(gpu)
    pos = torch.randint(0, 500, (T,), device=gpu)
    slots = torch.randperm(nb * bs, device=gpu)[:T]
    cs = ref.rope_cos_sin_cache(d, 1024, 5e5).to(gpu)
    kc = torch.zeros(nb, nkv, bs, d, dtype=FP8, device=gpu)
    vc = torch.zeros(nb, nkv, bs // 8, d, 8, dtype=FP8, device=gpu)
    kc2, vc2 = kc.cpu().clone(), vc.cpu().clone()
    ks, vs = scales
    q = ops.rope_kv_write(qkv, pos, cs, kc, vc, slots, nq, nkv, d, k_scale=ks, v_scale=vs)
    qr = ref.rope_qk_kv_write(qkv.cpu(), pos.cpu(), cs.cpu(), kc2, vc2, slots.cpu(), nq, nkv, d,
                              k_scale=ks, v_scale=vs)
    torch.testing.assert_close(q.cpu().float(), qr.float(), **_tol(dt))
    # V is a pure copy -> bit-exact; K passes through RoPE in fp32 first, so allow a
    # one-step (one fp8 ulp) disagreement on rounding ties of slightly different fp32
    assert torch.equal(vc.cpu().view(torch.uint8), vc2.view(torch.uint8))
    kd = (kc.cpu().view(torch.uint8).int() - kc2.view(torch.uint8).int()).abs()
    assert (kd > 1).sum() == 0 and (kd == 1).float().mean() < 0.01


def _fp8_cache(kc, vc, ks, vs):
    return (ref.to_cache(kc, FP8, ks), ref.to_cache(vc, FP8, vs))


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("d,nq,nkv", [(128, 32, 8), (64, 12, 12)])
def test_paged_decode_fp8(gpu, dt, d, nq, nkv):
    torch.manual_seed(13)
    ctx = [1, 33, 300, 1000, 2049]
    B, bs = len(ctx), 32
    kc, vc, bt = _fill_random_cache(B, ctx, nkv, bs, d, dt, gpu)
    ks, vs = 0.5, 2.0
    kc8, vc8 = _fp8_cache(kc, vc, ks, vs)
    q = torch.randn(B, nq, d, dtype=dt, device=gpu)
    cl = torch.tensor(ctx, dtype=torch.int32, device=gpu)
    for z in (1, 3):
        out = ops.paged_attention_decode(q, kc8, vc8, bt, cl, d ** -0.5, grid_z=z, k_scale=ks,
                                         v_scale=vs)
        exp = ref.paged_attention_decode(q.cpu(), kc8.cpu(), vc8.cpu(), bt.cpu(), cl.cpu(),
                                         d ** -0.5, ks, vs)
        torch.testing.assert_close(out.cpu().float(), exp.float(), **_tol(dt))


@pytest.mark.parametrize("dt", DT)
def test_prefill_attention_fp8(gpu, dt):
    torch.manual_seed(14)
    d, nq, nkv, bs = 128, 32, 8, 16
    seq_lens, query_lens = [5, 300, 700], [5, 100, 257]
    kc, vc, bt = _fill_random_cache(len(seq_lens), seq_lens, nkv, bs, d, dt, gpu)
    ks, vs = 1.0, 0.25
    kc8, vc8 = _fp8_cache(kc, vc, ks, vs)
    qsl = [0]
    for ql in query_lens:
        qsl.append(qsl[-1] + ql)
    q = torch.randn(qsl[-1], nq, d, dtype=dt, device=gpu)
    qsl_t = torch.tensor(qsl, dtype=torch.int32, device=gpu)
    sl_t = torch.tensor(seq_lens, dtype=torch.int32, device=gpu)
    out = ops.prefill_attention(q, kc8, vc8, bt, qsl_t, sl_t, d ** -0.5, k_scale=ks, v_scale=vs)
    exp = ref.prefill_attention(q.cpu(), kc8.cpu(), vc8.cpu(), bt.cpu(), qsl_t.cpu(), sl_t.cpu(),
                                d ** -0.5, ks, vs)
    torch.testing.assert_close(out.cpu().float(), exp.float(), **_tol(dt))


@pytest.mark.parametrize("M", [1, 5, 16])
@pytest.mark.parametrize("nt_o,nw", [(1, 4), (2, 8)])
def test_skinny_norm_free_pair(gpu, M, nt_o, nw):
    """K9 SK_ACC_SS then SK_RSCALE / SK_RSCALE_SILU == residual add, RMSNorm, GEMM in fp32:
    the producer's per-workgroup sums of squares of the stored residual, the consumer's
    row scale on the gamma-folded weight (plain and SiLU-pair outputs)."""
    from kubernetes_gpu_cluster_amd.ops import gemm
    torch.manual_seed(M + nt_o)
    dt, H, Kin, N, I = torch.bfloat16, 4096, 1024, 512, 256
    res = torch.randn(M, H, device=gpu).to(dt)
    x = (torch.randn(M, Kin, device=gpu) * 0.5).to(dt)
    wo = (torch.randn(H, Kin, device=gpu) * 0.03).to(dt)
    gamma = (torch.rand(H, device=gpu) + 0.5).to(dt)
    w = (torch.randn(N, H, device=gpu) * 0.02).to(dt)
    wgu = (torch.randn(2 * I, H, device=gpu) * 0.02).to(dt)
    ssp = torch.full((16 * 256,), float("nan"), device=gpu)
    r_ref = (res.float() + x.float() @ wo.float().t()).to(dt)
    nss = gemm.skinny_acc_ss(res, x, wo, (1, nt_o, nw, False), ssp)
    assert nss == H // (16 * nt_o)
    torch.testing.assert_close(res.float(), r_ref.float(), atol=2e-2, rtol=1e-2)
    ss = ssp[: M * nss].view(M, nss).sum(1)
    torch.testing.assert_close(ss, res.float().pow(2).sum(1), rtol=1e-4, atol=1e-3)
    inv = torch.rsqrt(res.float().pow(2).mean(1, keepdim=True) + 1e-5)
    normed = res.float() * inv * gamma.float()
    out = torch.empty(M, N, dtype=dt, device=gpu)
    gemm.skinny_rscale(res, gemm.fold_norm_weight(w, gamma), (1, 1, 4, False), ssp, nss, 1e-5,
                       out)
    torch.testing.assert_close(out.float(), normed @ w.float().t(), atol=3e-2, rtol=2e-2)
    act = torch.empty(M, I, dtype=dt, device=gpu)
    gemm.skinny_rscale(res, gemm.fold_norm_weight(wgu, gamma), (1, 2, 4, False), ssp, nss,
                       1e-5, act, silu=True)
    gu = normed @ wgu.float().t()
    exp = torch.nn.functional.silu(gu[:, :I]) * gu[:, I:]
    torch.testing.assert_close(act.float(), exp, atol=3e-2, rtol=2e-2)


# ------------------------------------------------------------------ K9 skinny GEMM
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("M,N,K", [(1, 6144, 4096), (7, 4096, 14336), (16, 512, 1024),
                                   (24, 1024, 2048), (33, 2048, 512), (64, 256, 4096)])
def test_skinny_gemm(gpu, dt, M, N, K):
    from kubernetes_gpu_cluster_amd.ops import gemm
    torch.manual_seed(M + N)
    x = torch.randn(M, K, dtype=dt, device=gpu)
    w = torch.randn(N, K, dtype=dt, device=gpu) * K ** -0.5
    b = torch.randn(N, dtype=dt, device=gpu)
    exp = x.float().cpu() @ w.float().cpu().t()
    mt = 1 if M <= 16 else (2 if M <= 32 else 4)
    for nt in (1, 2):
        for nw in (4, 8, 16):
            for ntl in (True, False):
                cfg = (mt, nt, nw, ntl)
                if not gemm.skinny_ok(M, N, K, cfg):
                    continue
                got = gemm.skinny_gemm(x, w, None, cfg)
                torch.testing.assert_close(got.float().cpu(), exp, atol=3e-2, rtol=2e-2)
                gotb = gemm.skinny_gemm(x, w, b, cfg)
                torch.testing.assert_close(gotb.float().cpu(), exp + b.float().cpu(), atol=3e-2,
                                           rtol=2e-2)


def test_skinny_gemm_strided_x(gpu):
    """X may be a row-strided view (e.g. a slice of a wider activation)."""
    from kubernetes_gpu_cluster_amd.ops import gemm
    torch.manual_seed(3)
    big = torch.randn(8, 3072, dtype=torch.bfloat16, device=gpu)
    x = big[:, :1024]
    w = torch.randn(512, 1024, dtype=torch.bfloat16, device=gpu) * 0.03
    got = gemm.skinny_gemm(x, w, None, (1, 1, 4, True))
    exp = x.float().cpu() @ w.float().cpu().t()
    torch.testing.assert_close(got.float().cpu(), exp, atol=3e-2, rtol=2e-2)


@pytest.mark.parametrize("M", [1, 5, 16])
@pytest.mark.parametrize("nw", [4, 16])
def test_skinny_gemm_norm_and_accumulate(gpu, M, nw):
    """K9 epilogues: SK_NORM == rms_norm(x) * gamma then the GEMM (+ bias);
    SK_ACC == C + x W^T (+ bias), in place."""
    from kubernetes_gpu_cluster_amd.ops import gemm
    torch.manual_seed(M * 7 + nw)
    K, N, eps = 2048, 512, 1e-5
    x = torch.randn(M, K, dtype=torch.bfloat16, device=gpu) * 3
    w = torch.randn(N, K, dtype=torch.bfloat16, device=gpu) * K ** -0.5
    g = (torch.rand(K, device=gpu) + 0.5).to(torch.bfloat16)
    b = torch.randn(N, dtype=torch.bfloat16, device=gpu)
    cfg = (1, 2, nw, True)
    xf, wf = x.float().cpu(), w.float().cpu()
    xn = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * g.float().cpu()
    got = gemm.skinny_norm(x, w, b, g, eps, cfg)
    torch.testing.assert_close(got.float().cpu(), xn @ wf.t() + b.float().cpu(), atol=3e-2,
                               rtol=2e-2)
    c0 = torch.randn(M, N, dtype=torch.bfloat16, device=gpu)
    exp = c0.float().cpu() + xf @ wf.t() + b.float().cpu()
    c = c0.clone()
    assert gemm.skinny_accum(c, x, w, b, cfg) is c
    torch.testing.assert_close(c.float().cpu(), exp, atol=6e-2, rtol=2e-2)


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("M,N,K", [(1, 28672, 4096), (5, 1024, 2048), (16, 2048, 1024),
                                   (40, 512, 4096), (64, 1024, 512)])
def test_skinny_silu_matches_fp32(gpu, dt, M, N, K):
    """K9 SK_SILU: silu(x Wg^T) * (x Wu^T) over a merged [gate; up] weight [2I, K] in one
    launch, every (mt, nw, ntl) holding M, vs fp32; and linear_silu takes the plan."""
    from kubernetes_gpu_cluster_amd.ops import gemm
    torch.manual_seed(M + N + K)
    x = torch.randn(M, K, dtype=dt, device=gpu)
    w = torch.randn(N, K, dtype=dt, device=gpu) * K ** -0.5
    ref = x.float().cpu() @ w.float().cpu().t()
    exp = torch.nn.functional.silu(ref[:, : N // 2]) * ref[:, N // 2:]
    ran = 0
    for cfg in gemm._CONFIGS:
        if cfg[1] != 2 or not gemm.skinny_ok(M, N, K, cfg):
            continue
        out = torch.full((M, N // 2), float("nan"), dtype=dt, device=gpu)
        gemm.skinny_silu(x, w, cfg, out)
        torch.testing.assert_close(out.float().cpu(), exp, atol=3e-2, rtol=2e-2)
        ran += 1
    assert ran > 0
    try:
        gemm._plan_silu[(M, N, K)] = (1 if M <= 16 else (2 if M <= 32 else 4), 2, 4, True)
        torch.testing.assert_close(gemm.linear_silu(x, w).float().cpu(), exp, atol=3e-2,
                                   rtol=2e-2)
    finally:
        gemm.clear_plan()


def test_tune_skinny_silu_records_plan(gpu):
    """The tuner times SK_SILU against the plain plan + silu_mul for merged gate_up shapes."""
    from kubernetes_gpu_cluster_amd.ops import gemm
    torch.manual_seed(9)
    ws = [torch.randn(4096, 2048, dtype=torch.bfloat16, device=gpu) * 0.02 for _ in range(4)]
    try:
        gemm.tune_skinny(ws, [1, 8], silu_shapes={(4096, 2048)})
        x = torch.randn(8, 2048, dtype=torch.bfloat16, device=gpu)
        ref = x.float() @ ws[0].float().t()
        exp = torch.nn.functional.silu(ref[:, :2048]) * ref[:, 2048:]
        torch.testing.assert_close(gemm.linear_silu(x, ws[0]).float(), exp, atol=3e-2, rtol=2e-2)
    finally:
        gemm.clear_plan()


def test_tune_skinny_times_norm_free_epilogues(gpu):
    """With rs_shapes the tuner times SK_ACC_SS (tail shapes), SK_RSCALE (norm shapes) and
    SK_RSCALE_SILU (merged gate_up) themselves at M <= 16, and rs_plan takes those
    configurations -- each one a form the norm-free layer can run (one m-tile,
    M <= 4 * NW, SiLU pairs at NT = 2)."""
    from kubernetes_gpu_cluster_amd.ops import gemm
    torch.manual_seed(10)
    shapes = [(768, 512), (512, 512), (2048, 512), (512, 1024)]   # qkv, o, gate_up, down
    ws = [torch.randn(n, k, dtype=torch.bfloat16, device=gpu) * 0.02
          for n, k in shapes for _ in range(2)]
    try:
        gemm.tune_skinny(ws, [1, 8], norm_shapes={shapes[0], shapes[2]},
                         silu_shapes={shapes[2]}, tail_shapes={shapes[1], shapes[3]},
                         rs_shapes=True)
        for M in (1, 8):
            plan = gemm.rs_plan(M, shapes)
            assert plan is not None
            want = [gemm._best_rs[("rs", M) + shapes[0]], gemm._best_rs[("ss", M) + shapes[1]],
                    gemm._best_rs[("rss", M) + shapes[2]], gemm._best_rs[("ss", M) + shapes[3]]]
            assert plan == want
            assert all(c[0] == 1 and M <= 4 * c[2] for c in plan) and plan[2][1] == 2
    finally:
        gemm.clear_plan()
    assert not gemm._best_rs


@pytest.mark.parametrize("cfg", list(range(15)))
@pytest.mark.parametrize("M,N,K", [(256, 1024, 4096), (200, 768, 1024), (77, 512, 2048),
                                   (130, 256, 128), (256, 1280, 1024), (200, 1792, 512),
                                   (96, 896, 256), (256, 1536, 2048)])
def test_dgemm_matches_fp32(gpu, cfg, M, N, K):
    """K9m decode GEMM (every tile config, packed and row-major weights) vs an fp32
    matmul: bf16 output (S = 1), fp32 split-K slices (S = 2, 3, 4, 5: uneven K ranges at 3
    and 5; 16 where K allows: the TP = 8 qkv split) and the fused SiLU epilogue where the
    tile has it, with M not a multiple of the row block (clamped loads, masked stores).
    The round-6 narrow tiles (11-14: BN 64 / 80 / 112, one or two waves along N, 128-row
    blocks XCD-paired) read pieces of the 128-row packed blocks; N = 1280 / 1792 / 896 put
    their column tiles across those blocks' boundaries."""
    from kubernetes_gpu_cluster_amd.ops import gemm
    k = torch.ops.kgc
    assert k.dgemm_num_cfgs() == 15
    bm, bn, pk = k.dgemm_cfg_info(cfg)
    if N % bn:
        pytest.skip("N not a multiple of BN")
    epis = k.dgemm_cfg_epis(cfg)
    torch.manual_seed(M + N + cfg)
    x = torch.randn(M, K, dtype=torch.bfloat16, device=gpu)
    w = torch.randn(N, K, dtype=torch.bfloat16, device=gpu) * 0.02
    ref = x.float().cpu() @ w.float().cpu().t()

    def weight(silu):
        if not pk:
            return w
        p = torch.empty(N // 128, K // 64, 8192, dtype=w.dtype, device=gpu)
        k.dgemm_pack(p, w, silu)
        return p
    out = torch.empty(M, N, dtype=torch.bfloat16, device=gpu)
    k.dgemm(out, x, weight(False), cfg, 1)
    torch.testing.assert_close(out.float().cpu(), ref, atol=3e-2, rtol=2e-2)
    for S in (s for s in (2, 3, 4, 5, 16) if s <= K // 64):
        ws = torch.full((S, M, N), float("nan"), dtype=torch.float32, device=gpu)
        k.dgemm(ws, x, weight(False), cfg, 0)
        # every slice row was written (no NaN left) and the slices sum to the product
        torch.testing.assert_close(ws.sum(0).cpu(), ref, atol=2e-3, rtol=2e-3)
    act = torch.empty(M, N // 2, dtype=torch.bfloat16, device=gpu)
    if not (epis >> 2) & 1:
        with pytest.raises(RuntimeError, match="no such epilogue"):
            k.dgemm(act, x, weight(True), cfg, 2)
        return
    k.dgemm(act, x, weight(True), cfg, 2)
    exp = torch.nn.functional.silu(ref[:, : N // 2]) * ref[:, N // 2:]
    torch.testing.assert_close(act.float().cpu(), exp, atol=3e-2, rtol=2e-2)
    # the SiLU-packed weight's fp32 slices, reduced by splitk_reduce_silu (interleaved
    # gate / up 16-column groups in packed tiles): the split-K path of gate_up
    if K // 64 >= 4:
        ws = torch.empty(4, M, N, dtype=torch.float32, device=gpu)
        k.dgemm(ws, x, weight(True), cfg, 0)
        red = torch.empty(M, N // 2, dtype=torch.bfloat16, device=gpu)
        k.splitk_reduce_silu(red, ws, bool(pk))
        torch.testing.assert_close(red.float().cpu(), exp, atol=3e-2, rtol=2e-2)


def test_dgemm_pack_layout(gpu):
    """The packed tile [nb][kb][r][pos] holds W[nb*128 + r][kb*64 + (pos ^ r%8)*8 ..]."""
    k = torch.ops.kgc
    N, K = 256, 128
    w = torch.arange(N * K, dtype=torch.float32).reshape(N, K).to(torch.float16).to(gpu)
    p = torch.empty(N // 128, K // 64, 8192, dtype=w.dtype, device=gpu)
    k.dgemm_pack(p, w, False)
    pc = p.cpu().view(N // 128, K // 64, 128, 8, 8)
    wc = w.cpu()
    for nb, kb, r, pos in [(0, 0, 0, 0), (1, 1, 5, 3), (0, 1, 127, 7), (1, 0, 64, 2)]:
        src = wc[nb * 128 + r, kb * 64 + (pos ^ (r % 8)) * 8: kb * 64 + (pos ^ (r % 8)) * 8 + 8]
        assert torch.equal(pc[nb, kb, r, pos], src)


def test_linear_uses_dgemm_plan(gpu):
    from kubernetes_gpu_cluster_amd.ops import gemm
    torch.manual_seed(5)
    w = torch.randn(1024, 4096, dtype=torch.bfloat16, device=gpu) * 0.02
    x = torch.randn(96, 4096, dtype=torch.bfloat16, device=gpu)
    assert gemm.pack_decode_weights([w], []) > 0
    try:
        for plan in [(5, 4), (2, 1), (6, 2)]:
            gemm._plan_dg[(96, 1024, 4096, "plain")] = plan
            got = gemm.linear(x, w)
            torch.testing.assert_close(got.float(), (x.float() @ w.float().t()), atol=3e-2,
                                       rtol=2e-2)
    finally:
        gemm.clear_plan()
        gemm._packed.clear()


def test_linear_uses_tuned_plan(gpu):
    from kubernetes_gpu_cluster_amd.ops import gemm
    torch.manual_seed(4)
    ws = [torch.randn(1024, 2048, dtype=torch.bfloat16, device=gpu) * 0.02 for _ in range(4)]
    res = gemm.tune_skinny(ws, [1, 8, 64])
    assert set(res) == {(1, 1024, 2048), (8, 1024, 2048), (64, 1024, 2048)}
    x = torch.randn(8, 2048, dtype=torch.bfloat16, device=gpu)
    torch.testing.assert_close(gemm.linear(x, ws[0]).float(), (x @ ws[0].t()).float(),
                               atol=3e-2, rtol=2e-2)
    gemm.clear_plan()



@pytest.mark.parametrize("M,N,K,plan", [(256, 2048, 4096, (8, 1)), (80, 1536, 2048, (5, 1)),
                                         (144, 1024, 1024, (0, 2)), (96, 2048, 2048, (2, 1)),
                                         (256, 2048, 4096, (4, 2)), (256, 7168, 1024, (6, 5)),
                                         (200, 1024, 2048, (9, 3)), (256, 2048, 4096, (6, 1))])
def test_linear_silu_dgemm_matches_fp32(gpu, M, N, K, plan):
    """gate_up through the K9m plan -- fused SiLU epilogue (S = 1, packed silu weights) or
    split-K slices summed by splitk_reduce_silu (row-major tiles: [gate | up] halves; packed
    tiles: the interleaved 16-column groups of the SiLU packing) -- vs an fp32 silu(g) * u
    reference.  Only the SiLU-packed copy exists, as in the engine."""
    from kubernetes_gpu_cluster_amd.ops import gemm
    torch.manual_seed(M + N + 1)
    x = torch.randn(M, K, dtype=torch.bfloat16, device=gpu)
    w = torch.randn(N, K, dtype=torch.bfloat16, device=gpu) * 0.03
    y = x.float().cpu() @ w.float().cpu().t()
    ref = torch.nn.functional.silu(y[:, : N // 2]) * y[:, N // 2:]
    gemm.pack_decode_weights([], [w])
    gemm._plan_dg[(M, N, K, "silu")] = plan
    try:
        got = gemm.linear_silu(x, w)
    finally:
        gemm.clear_plan()
        gemm._packed.clear()
    assert got.shape == (M, N // 2)
    torch.testing.assert_close(got.float().cpu(), ref, atol=3e-2, rtol=2e-2)


@pytest.mark.parametrize("M,N,K,plan", [(256, 4096, 4096, (6, 4)), (96, 4096, 14336, (5, 8)),
                                         (130, 1024, 2048, (4, 1))])
def test_linear_add_rms_dgemm_matches_fp32(gpu, M, N, K, plan):
    """K9m split-K reduction fused into residual add + RMSNorm vs an fp32 reference of
    residual += x W^T; out = rms_norm(residual) * gamma."""
    from kubernetes_gpu_cluster_amd.ops import gemm
    torch.manual_seed(M + K)
    x = torch.randn(M, K, dtype=torch.bfloat16, device=gpu)
    w = torch.randn(N, K, dtype=torch.bfloat16, device=gpu) * 0.02
    res = torch.randn(M, N, dtype=torch.bfloat16, device=gpu)
    gamma = torch.rand(N, dtype=torch.bfloat16, device=gpu) + 0.5
    r32 = res.float().cpu() + (x.float().cpu() @ w.float().cpu().t())
    exp = r32 * torch.rsqrt(r32.pow(2).mean(-1, keepdim=True) + 1e-5) * gamma.float().cpu()
    gemm.pack_decode_weights([w], [])
    gemm._plan_dg[(M, N, K, "tail")] = plan
    try:
        out, r = gemm.linear_add_rms(x, w, res, gamma, 1e-5)
    finally:
        gemm.clear_plan()
        gemm._packed.clear()
    assert r.data_ptr() == res.data_ptr()   # residual updated in place
    torch.testing.assert_close(r.float().cpu(), r32, atol=5e-2, rtol=2e-2)
    torch.testing.assert_close(out.float().cpu(), exp, atol=5e-2, rtol=2e-2)


def test_tail_fused_model_matches_regular_path(gpu):
    """Whole-model forward with o/down reductions fused into the norms (forced K9m split-K
    plan) vs the regular layer loop on the same weights."""
    from kubernetes_gpu_cluster_amd.models import configs
    from kubernetes_gpu_cluster_amd.models.llama import LlamaForCausalLM
    from kubernetes_gpu_cluster_amd.ops import gemm
    from kubernetes_gpu_cluster_amd.models import llama as llama_mod
    cfg = configs.PRESETS["llama-3-8b"].shrink(name="tail-fuse", num_layers=2)
    torch.manual_seed(0)
    model = LlamaForCausalLM(cfg, torch.bfloat16, gpu)
    for p in model.parameters():
        p.data.normal_(0, 0.02) if p.dim() == 2 else p.data.fill_(1.0)
    M = 96
    ids = torch.randint(0, cfg.vocab_size, (M,), device=gpu)
    x = model.embed_tokens(ids)

    class _Ctx:
        pass
    # exercise the projection tail only: attention replaced by an identity-shaped stub
    for l in model.layers:
        l.self_attn.attend = (lambda positions, qkv, ctx, nq=l.self_attn.nq * cfg.head_dim:
                              qkv[:, :nq].contiguous())
    ref_out = None
    try:
        llama_mod._tail_fusion_enabled = False
        ref_out = model(ids, None, _Ctx())
        for l in model.layers:
            for w in (l.self_attn.o_proj.weight, l.mlp.down_proj.weight):
                gemm._plan_dg[(M, w.shape[0], w.shape[1], "tail")] = (2, 4)
        llama_mod._tail_fusion_enabled = True
        assert model._tail_fusable(x)
        got = model(ids, None, _Ctx())
    finally:
        gemm.clear_plan()
        llama_mod._tail_fusion_enabled = True
    torch.testing.assert_close(got.float(), ref_out.float(), atol=6e-2, rtol=3e-2)


@pytest.mark.parametrize("M,N,K,cfg,S", [(256, 4096, 2048, 6, 1), (96, 2048, 1024, 5, 1),
                                         (256, 2048, 1024, 4, 3), (100, 1024, 1024, 2, 2),
                                         (256, 1024, 1024, 0, 1)])
def test_dgemm_row_scale_silu_matches_fp32(gpu, M, N, K, cfg, S):
    """The K9m row-scale epilogue: silu(r * g) * (r * u) over a merged gate_up weight, r per
    row -- in the SiLU epilogue (S = 1) or in splitk_reduce_silu (S > 1) -- vs fp32; and
    the EPI_OUT row scale."""
    from kubernetes_gpu_cluster_amd.ops import gemm
    torch.manual_seed(M + K)
    x = torch.randn(M, K, dtype=torch.bfloat16, device=gpu)
    w = torch.randn(N, K, dtype=torch.bfloat16, device=gpu) * K ** -0.5
    r = torch.rand(M, dtype=torch.float32, device=gpu) + 0.5
    y = (x.float().cpu() @ w.float().cpu().t()) * r.cpu()[:, None]
    ref = torch.nn.functional.silu(y[:, : N // 2]) * y[:, N // 2:]
    pk = gemm.cfg_packed(cfg)

    def packed(silu):
        if not pk:
            return w
        p = torch.empty(N // 128, K // 64, 8192, dtype=w.dtype, device=gpu)
        torch.ops.kgc.dgemm_pack(p, w, silu)
        return p
    wk = packed(True)
    if S == 1:
        got = gemm.dgemm(x, w, cfg, 1, epi=2, rscale=r, wk=wk)
    else:
        got = torch.empty(M, N // 2, dtype=x.dtype, device=gpu)
        torch.ops.kgc.splitk_reduce_silu(got, gemm.dgemm(x, w, cfg, S, wk=wk), pk, r)
    torch.testing.assert_close(got.float().cpu(), ref, atol=3e-2, rtol=2e-2)
    out = gemm.dgemm(x, w, cfg, 1, epi=1, rscale=r, wk=packed(False))
    torch.testing.assert_close(out.float().cpu(), y, atol=3e-2, rtol=2e-2)


@pytest.mark.parametrize("S", [0, 4, 5])
def test_paged_decode_rope_row_scale(gpu, monkeypatch, S):
    """The fused decode-attention prologue with the norm-free row scale: slices (or the bf16
    projection) scaled per row inside the kernel == the same kernel fed the pre-scaled
    projection, for the attention output and the written K / V."""
    torch.manual_seed(S + 3)
    B, nq, nkv, d, bs = 96, 32, 8, 128, 32
    N = (nq + 2 * nkv) * d
    ctx_len = 200
    nblk = (ctx_len + bs - 1) // bs
    kc0 = torch.randn(B * nblk + 1, nkv, bs, d, dtype=torch.bfloat16, device=gpu) * 0.5
    vc0 = torch.randn(B * nblk + 1, nkv, bs // 8, d, 8, dtype=torch.bfloat16, device=gpu) * 0.5
    bt = (torch.arange(B * nblk, dtype=torch.int32, device=gpu) + 1).view(B, nblk)
    cl = torch.full((B,), ctx_len, dtype=torch.int32, device=gpu)
    pos = (cl - 1).to(torch.int64)
    slots = (bt[:, (ctx_len - 1) // bs].to(torch.int64) * bs + (ctx_len - 1) % bs)
    cs = torch.randn(4096, d, dtype=torch.float32, device=gpu)
    r = torch.rand(B, dtype=torch.float32, device=gpu) + 0.5
    if S:
        sl = torch.randn(S, B, N, dtype=torch.float32, device=gpu) * 0.5
        pre = (sl.sum(0) * r[:, None]).to(torch.bfloat16)
        raw = sl
    else:
        raw = torch.randn(B, N, dtype=torch.bfloat16, device=gpu)
        pre = (raw.float() * r[:, None]).to(torch.bfloat16)

    def run(qkv, rsc):
        kc, vc = kc0.clone(), vc0.clone()
        o = ops.paged_attention_decode_rope(qkv, pos, cs, kc, vc, slots, nq, nkv, d, bt, cl,
                                            d ** -0.5, dtype=torch.bfloat16, row_scale=rsc)
        return o, kc, vc
    o1, k1, v1 = run(raw, r)
    o2, k2, v2 = run(pre, None)
    torch.testing.assert_close(o1.float(), o2.float(), atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(k1.float(), k2.float(), atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(v1.float(), v2.float(), atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("M,N,K,cfg", [(1, 4096, 4096, (1, 1, 4, True)),
                                       (5, 4096, 14336, (1, 2, 8, False)),
                                       (16, 1024, 2048, (1, 1, 16, True)),
                                       (40, 512, 1024, (4, 2, 4, False))])
def test_skinny_acc_norm_matches_fp32(gpu, M, N, K, cfg):
    """K9 SK_ACC_NORM: residual += x W^T, then out = rms_norm(residual) * gamma by the last
    workgroup of the same launch, vs fp32; repeated eager calls and graph replays re-arm
    the ticket (every call normalises, none is skipped)."""
    from kubernetes_gpu_cluster_amd.ops import gemm
    torch.manual_seed(M + N)
    x = torch.randn(M, K, dtype=torch.bfloat16, device=gpu)
    w = torch.randn(N, K, dtype=torch.bfloat16, device=gpu) * K ** -0.5
    res0 = torch.randn(M, N, dtype=torch.bfloat16, device=gpu)
    gamma = torch.rand(N, dtype=torch.bfloat16, device=gpu) + 0.5

    def expect(r_before):
        r32 = r_before.float().cpu() + x.float().cpu() @ w.float().cpu().t()
        return r32, r32 * torch.rsqrt(r32.pow(2).mean(-1, keepdim=True) + 1e-5) * gamma.float().cpu()
    res = res0.clone()
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=gpu)
    for _ in range(3):
        before = res.clone()
        gemm.skinny_acc_norm(res, x, w, gamma, 1e-5, cfg, out)
        r32, exp = expect(before)
        torch.testing.assert_close(res.float().cpu(), r32, atol=5e-2, rtol=2e-2)
        # normalised from the bf16 residual as stored: compare against that exactly-rounded row
        rb = res.float().cpu()
        exact = (rb * torch.rsqrt(rb.pow(2).mean(-1, keepdim=True) + 1e-5) * gamma.float().cpu())
        torch.testing.assert_close(out.float().cpu(), exact, atol=2e-2, rtol=1e-2)
        torch.testing.assert_close(out.float().cpu(), exp, atol=6e-2, rtol=3e-2)
    assert int(gemm._ticket(x.device)[0]) == 0
    g = torch.cuda.CUDAGraph()
    res.copy_(res0)
    with torch.cuda.graph(g):
        gemm.skinny_acc_norm(res, x, w, gamma, 1e-5, cfg, out)
    for _ in range(2):
        res.copy_(res0)
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        _, exp = expect(res0)
        torch.testing.assert_close(out.float().cpu(), exp, atol=6e-2, rtol=3e-2)
    assert int(gemm._ticket(x.device)[0]) == 0


def test_tail_fused_model_small_m_acc_norm(gpu):
    """Whole-model forward at M = 4 with o/down + the consuming norms as SK_ACC_NORM
    launches (forced plan) vs the regular layer loop on the same weights."""
    from kubernetes_gpu_cluster_amd.models import configs
    from kubernetes_gpu_cluster_amd.models.llama import LlamaForCausalLM
    from kubernetes_gpu_cluster_amd.ops import gemm
    from kubernetes_gpu_cluster_amd.models import llama as llama_mod
    cfg = configs.PRESETS["llama-3-8b"].shrink(name="tail-fuse-s", num_layers=2)
    torch.manual_seed(1)
    model = LlamaForCausalLM(cfg, torch.bfloat16, gpu)
    for p in model.parameters():
        p.data.normal_(0, 0.02) if p.dim() == 2 else p.data.fill_(1.0)
    M = 4
    ids = torch.randint(0, cfg.vocab_size, (M,), device=gpu)
    x = model.embed_tokens(ids)

    class _Ctx:
        pass
    for l in model.layers:
        l.self_attn.attend = (lambda positions, qkv, ctx, nq=l.self_attn.nq * cfg.head_dim:
                              qkv[:, :nq].contiguous())
    try:
        llama_mod._tail_fusion_enabled = False
        ref_out = model(ids, None, _Ctx())
        for l in model.layers:
            for w in (l.self_attn.o_proj.weight, l.mlp.down_proj.weight):
                gemm._plan_accnorm[(M, w.shape[0], w.shape[1])] = (1, 1, 8, True)
        llama_mod._tail_fusion_enabled = True
        assert model._tail_fusable(x)
        got = model(ids, None, _Ctx())
    finally:
        gemm.clear_plan()
        llama_mod._tail_fusion_enabled = True
    torch.testing.assert_close(got.float(), ref_out.float(), atol=6e-2, rtol=3e-2)


def test_sampler_health_word(gpu):
    """The cooperative sampler's sticky barrier-timeout word: zero after a normal top-k /
    top-p step, copied and cleared behind the step, and a set word raises SamplerFailed."""
    torch.manual_seed(0)
    B, V = 8, 32000
    logits = torch.randn(B, V, device=gpu)
    sh = ops.SamplerHealth(gpu)
    temp = torch.full((B,), 0.8, device=gpu)
    topk = torch.full((B,), 40, dtype=torch.int32, device=gpu)
    topp = torch.full((B,), 0.9, device=gpu)
    seeds = torch.arange(B, dtype=torch.int64, device=gpu)
    ops.sample(logits, temp, topk, topp, seeds)
    slot = sh.enqueue_err_read()
    torch.cuda.synchronize()
    sh.raise_if_failed(slot)                      # healthy step: no error
    sh.host[slot] = 1
    with pytest.raises(ops.SamplerFailed):
        sh.raise_if_failed(slot)
    assert int(sh.host[slot]) == 0


def test_sampler_health_async_steps_keep_their_flags(gpu):
    """Async scheduling launches step N + 1 before step N's tokens are read: step N's
    failure (its word set) must still be reported for N, although N + 1's copy of the
    then-cleared word lands later -- each step copies into its own host slot."""
    k = torch.ops.kgc
    sh = ops.SamplerHealth(gpu)
    k.u32_fill_async(sh.addr, 1)                  # step N: the barrier timed out
    slot_n = sh.enqueue_err_read()                # ... its copy, then the clear
    slot_n1 = sh.enqueue_err_read()               # step N + 1: healthy (word now 0)
    torch.cuda.synchronize()                      # both copies landed (N + 1's last)
    sh.raise_if_failed(slot_n1)                   # N + 1 is fine ...
    with pytest.raises(ops.SamplerFailed):        # ... and N is still reported
        sh.raise_if_failed(slot_n)


def test_dg_table_fingerprint_guards_stale_tables(gpu, tmp_path, monkeypatch):
    """an offline K9m table is trusted only when its fingerprint (GPU arch and
    CU count, the library's tile-config list) matches the running build; a mismatching or
    unfingerprinted table is dropped whole (start-up tuning runs), and an entry whose tile
    does not divide its N or whose split exceeds K / 64 is dropped alone."""
    import json
    from kubernetes_gpu_cluster_amd.ops import gemm
    fp = gemm.dg_fingerprint()
    assert fp["num_cfgs"] == torch.ops.kgc.dgemm_num_cfgs() and len(fp["cfgs"]) == fp["num_cfgs"]
    ent = [{"M": 256, "N": 4096, "K": 4096, "kind": "tail", "cfg": 6, "S": 4},
           {"M": 256, "N": 1280, "K": 8192, "kind": "plain", "cfg": 6, "S": 4},   # 1280 % 128 ok
           {"M": 256, "N": 1280, "K": 8192, "kind": "qkv", "cfg": 12, "S": 16},   # BN 80
           {"M": 256, "N": 1280, "K": 1024, "kind": "tail", "cfg": 12, "S": 32},  # S > K/64
           {"M": 256, "N": 1000, "K": 4096, "kind": "plain", "cfg": 4, "S": 1}]   # N % BN
    path = tmp_path / "t.json"
    monkeypatch.setenv("KGC_DGEMM_TABLE", str(path))
    try:
        path.write_text(json.dumps({"fingerprint": fp, "entries": ent}))
        assert gemm.load_dg_table("x") == 3
        bad = dict(fp, cfgs=fp["cfgs"][:-1], num_cfgs=fp["num_cfgs"] - 1)
        path.write_text(json.dumps({"fingerprint": bad, "entries": ent}))
        assert gemm.load_dg_table("x") == 0
        path.write_text(json.dumps({"fingerprint": dict(fp, arch="gfx942"), "entries": ent}))
        assert gemm.load_dg_table("x") == 0
        path.write_text(json.dumps({"fingerprint": dict(fp, cus=fp["cus"] // 2), "entries": ent}))
        assert gemm.load_dg_table("x") == 0
        # the marketing name is informational: libdrm resolves it differently under
        # rocprofv3, and a profiled run must load the same table as the service runs
        path.write_text(json.dumps({"fingerprint": dict(fp, device="AMD Radeon Graphics (x)"),
                                    "entries": ent}))
        assert gemm.load_dg_table("x") == 3
        path.write_text(json.dumps({"entries": ent}))
        assert gemm.load_dg_table("x") == 0
        # the committed table matches this library
        monkeypatch.delenv("KGC_DGEMM_TABLE")
        assert gemm.load_dg_table("llama-3-8b") > 0
    finally:
        gemm.clear_plan()
