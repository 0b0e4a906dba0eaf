"""K9mf's host side without a GPU: the packed mxfp4 tile layout (ops/quant.py
``pack_mxfp4_tiles_reference``), the shapes the kernel takes, and the CPU path of the
dispatcher with K9mf plan entries installed."""
import pytest
import torch

from kubernetes_gpu_cluster_amd.ops import gemm
from kubernetes_gpu_cluster_amd.ops.quant import (MXFP4_TILE_BYTES, attach_w4_scale,
                                                  dequantize_mxfp4, pack_mxfp4_tiles_reference,
                                                  quantize_mxfp4, tile_rows)


def _distinct(N, K):
    """Code and scale tensors filled with their own flat addresses.  A byte holds only 256
    distinct values, so ``_pack_addresses`` packs the addresses one byte plane at a time
    (the pack is a pure byte permutation) and reassembles them."""
    ca = torch.arange(N * K // 2, dtype=torch.int64).view(N, K // 2)
    sa = torch.arange(N * K // 32, dtype=torch.int64).view(N, K // 32)
    return ca, sa


def _pack_addresses(ca, sa, silu):
    """pack_mxfp4_tiles_reference applied to 24-bit addresses, one byte plane at a time."""
    out = None
    for shift in (0, 8, 16):
        p = pack_mxfp4_tiles_reference(((ca >> shift) & 0xFF).to(torch.uint8),
                                       ((sa >> shift) & 0xFF).to(torch.uint8), silu)
        out = p.to(torch.int64) << shift if out is None else out | (p.to(torch.int64) << shift)
    return out


def _index_map(N, K, silu):
    """The documented layout as explicit loops over tile bytes: (is_scale, source address)
    per packed byte, written independently of the reference's view / permute chain."""
    nb_n, nk = N // 128, K // 64
    rows = tile_rows(N, silu)
    is_scale = torch.zeros(nb_n, nk, MXFP4_TILE_BYTES, dtype=torch.bool)
    src = torch.zeros(nb_n, nk, MXFP4_TILE_BYTES, dtype=torch.int64)
    for nb in range(nb_n):
        for kb in range(nk):
            for r in range(128):
                wr = int(rows[nb, r])
                for pos in range(4):
                    q = pos ^ (2 * ((r // 8) % 2))
                    for half in range(2):
                        for e in range(4):
                            o = r * 32 + pos * 8 + half * 4 + e
                            src[nb, kb, o] = wr * (K // 2) + kb * 32 + half * 16 + q * 4 + e
            for wn in range(2):
                for r16 in range(16):
                    for n in range(4):
                        for ks in range(2):
                            o = 4096 + wn * 128 + r16 * 8 + n * 2 + ks
                            wr = int(rows[nb, wn * 64 + n * 16 + r16])
                            is_scale[nb, kb, o] = True
                            src[nb, kb, o] = wr * (K // 32) + kb * 2 + ks
    return is_scale, src


@pytest.mark.parametrize("silu", [False, True])
def test_pack_reference_is_a_permutation_and_follows_the_index_map(silu):
    N, K = 256, 192
    ca, sa = _distinct(N, K)
    p = _pack_addresses(ca, sa, silu)
    assert p.shape == (N // 128, K // 64, MXFP4_TILE_BYTES) and MXFP4_TILE_BYTES == 4352
    codes, scales = p[:, :, :4096].flatten(), p[:, :, 4096:].flatten()
    # every code byte and every scale byte lands exactly once, in its own region
    assert torch.equal(codes.sort().values, torch.arange(N * K // 2))
    assert torch.equal(scales.sort().values, torch.arange(N * K // 32))
    is_scale, src = _index_map(N, K, silu)
    assert bool(is_scale[:, :, 4096:].all()) and not bool(is_scale[:, :, :4096].any())
    assert torch.equal(p, src)
    # and on real bytes: a gather through the map reproduces the reference
    g = torch.Generator().manual_seed(0)
    w4, sc = quantize_mxfp4(torch.randn(N, K, generator=g))
    flat = torch.where(is_scale, sc.flatten()[src.clamp(max=sc.numel() - 1)],
                       w4.flatten()[src.clamp(max=w4.numel() - 1)])
    assert torch.equal(pack_mxfp4_tiles_reference(w4, sc, silu), flat)


def test_pack_reference_rejects_bad_shapes():
    w4, sc = quantize_mxfp4(torch.randn(128, 64))
    assert pack_mxfp4_tiles_reference(w4, sc).shape == (1, 1, 4352)
    assert pack_mxfp4_tiles_reference(w4, sc, silu=True).shape == (1, 1, 4352)
    with pytest.raises(AssertionError):
        pack_mxfp4_tiles_reference(w4, sc[:, :1])                # scales [N, K / 32]
    w4, sc = quantize_mxfp4(torch.randn(128, 96))
    with pytest.raises(AssertionError):
        pack_mxfp4_tiles_reference(w4, sc)                       # K % 64
    w4, sc = quantize_mxfp4(torch.randn(64, 64))
    with pytest.raises(AssertionError):
        pack_mxfp4_tiles_reference(w4, sc)                       # N % 128


def test_w4_dg_ok_rejects_what_the_kernel_cannot_run():
    ok = gemm.w4_dg_ok
    assert ok(65, 128, 64) and ok(512, 4096, 14336, 4, 32) and ok(256, 128, 1024, 0, 16)
    assert not ok(64, 128, 64) and not ok(513, 128, 64) and not ok(0, 128, 64)
    assert not ok(128, 64, 64) and not ok(128, 192, 64) and not ok(128, 0, 64)
    assert not ok(128, 128, 32) and not ok(128, 128, 96) and not ok(128, 128, 0)
    assert not ok(128, 128, 128, 0, 3)          # more slices than 64-k steps
    assert not ok(128, 128, 4096, 0, 33) and not ok(128, 128, 4096, 0, 0)
    assert not ok(128, 128, 4096, -1, 1)


def test_counts_and_plan_accessors():
    c = gemm.w4_counts()
    assert set(c) == {"k9f", "k9f_silu", "widen", "k9mf", "k9mf_silu"}
    gemm.clear_plan()
    try:
        gemm._plan_w4_dg[(96, 512, 1024, "tail")] = (2, 2)
        gemm._plan_w4_dg[(128, 512, 1024, "tail")] = None
        assert gemm.w4_dg_plan() == {(96, 512, 1024, "tail"): (2, 2),
                                     (128, 512, 1024, "tail"): None}
        assert gemm.tail_plan_has_m(96) and not gemm.tail_plan_has_m(128)
        assert not gemm.w4_plan()               # mid-bucket entries never reach w4_plan()
        gemm.clear_plan()
        assert not gemm.w4_dg_plan() and not gemm.tail_plan_has_m(96)
    finally:
        gemm.clear_plan()


def test_a_plan_entry_does_not_touch_the_cpu_path():
    g = torch.Generator().manual_seed(2)
    M, N, K = 96, 256, 128
    w = torch.randn(N, K, generator=g) * K ** -0.5
    w4, sc = quantize_mxfp4(w)
    attach_w4_scale(w4, sc)
    dq = dequantize_mxfp4(w4, sc)
    x = torch.randn(M, K, generator=g)
    res = torch.randn(M, N, generator=g)
    gamma = torch.rand(N, generator=g) + 0.5
    y = x @ dq.t()
    gemm.clear_plan()
    c0 = gemm.w4_counts()
    try:
        for kind in ("plain", "silu", "tail"):
            gemm._plan_w4_dg[(M, N, K, kind)] = (2, 2)
        torch.testing.assert_close(gemm.linear(x, w4), y)
        torch.testing.assert_close(gemm.linear_silu(x, w4),
                                   torch.nn.functional.silu(y[:, :N // 2]) * y[:, N // 2:])
        r = res.clone()
        nrm, r2 = gemm.linear_add_rms(x, w4, r, gamma, 1e-6)
        rn = res + y
        torch.testing.assert_close(r2, rn)
        torch.testing.assert_close(nrm, rn * torch.rsqrt(rn.pow(2).mean(-1, keepdim=True) + 1e-6)
                                   * gamma)
        assert gemm.w4_counts() == c0           # no GPU path was counted
        assert gemm.w4_packed_weight(w4) is None
        assert gemm.pack_w4_decode_weights([w4], []) == 0        # a CPU weight: nothing packed
    finally:
        gemm.clear_plan()
