"""``--quantization fp8`` at the decode buckets with 64 < M <= 512 (K9mq,
csrc/kernels/gemm_w8_decode.hip): the packed tile layout's plain-torch reference, the shape
checks and the dispatcher, on the CPU."""
import pytest
import torch

from kubernetes_gpu_cluster_amd.ops import gemm
from kubernetes_gpu_cluster_amd.ops.quant import pack_fp8_tiles_reference, quantize_fp8_rows

SWZ = (0, 2, 3, 1)


def _w8(N, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    return quantize_fp8_rows(torch.randn(N, K, generator=g) * K ** -0.5)


@pytest.mark.parametrize("silu", [False, True])
def test_pack_reference_is_a_permutation(silu):
    w8, _ = _w8(384, 192)
    p = pack_fp8_tiles_reference(w8, silu)
    assert p.dtype == torch.uint8 and p.shape == (3, 3, 8192)
    assert torch.equal(p.flatten().sort().values, w8.view(torch.uint8).flatten().sort().values)


def _packed_at(p, N, n, k, silu):
    """w8[n, k] looked up in the packed tiles, from the layout's description alone."""
    if silu:
        up, row = divmod(n, N // 2)            # gate (0) or up (1) half, row inside it
        nb, r64 = divmod(row, 64)              # a column tile holds 64 gate + 64 up rows
        r = ((r64 // 16) * 2 + up) * 16 + r64 % 16
    else:
        nb, r = divmod(n, 128)
    kb, kk = divmod(k, 64)
    half, k32 = divmod(kk, 32)                 # the first / second MFMA of the step
    q, e = divmod(k32, 8)
    pos = q ^ SWZ[(r // 4) % 4]
    return p[nb, kb, r * 64 + pos * 16 + half * 8 + e]


@pytest.mark.parametrize("silu", [False, True])
def test_pack_reference_gather(silu):
    N, K = 256, 192
    w8, _ = _w8(N, K, seed=1)
    raw = w8.view(torch.uint8)
    p = pack_fp8_tiles_reference(w8, silu)
    for n, k in [(0, 0), (5, 17), (19, 63), (127, 40), (128, 64), (130, 70), (200, 133),
                 (255, 191), (77, 100), (143, 8)]:
        assert _packed_at(p, N, n, k, silu) == raw[n, k], (silu, n, k)


def test_w8_dg_ok_rejects_what_the_kernel_cannot_run():
    assert gemm.w8_dg_ok(65, 128, 64, 0, 1)
    assert gemm.w8_dg_ok(512, 4096, 14336, 0, 8)
    assert not gemm.w8_dg_ok(64, 4096, 4096, 0, 1)            # M <= 64: K9q's
    assert not gemm.w8_dg_ok(513, 4096, 4096, 0, 1)           # M > 512
    assert not gemm.w8_dg_ok(128, 4096 + 64, 4096, 0, 1)      # N % 128
    assert not gemm.w8_dg_ok(128, 4096, 4096 + 32, 0, 1)      # K % 64
    assert not gemm.w8_dg_ok(128, 4096, 192, 0, 4)            # S > K / 64
    assert gemm.w8_dg_ok(128, 4096, 192, 0, 3)


def test_plan_entry_does_not_touch_the_cpu_path():
    M, N, K = 96, 256, 128
    w8, scale = _w8(N, K, seed=2)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16)
    exp = torch.nn.functional.linear(x, (w8.float() * scale[:, None]).to(torch.bfloat16))
    gemm._plan_w8_dg[(M, N, K, "plain")] = (0, 1)
    try:
        assert (M, N, K, "plain") in gemm.w8_dg_plan()
        assert torch.equal(gemm.linear(x, w8), exp)
    finally:
        gemm.clear_plan()
    assert not gemm.w8_dg_plan()
    assert {"k9mq", "k9mq_silu"} <= set(gemm.w8_counts())
