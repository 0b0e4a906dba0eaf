"""K1 (decode, plain and with RoPE / KV write folded in) and K2 (prefill) against the float64
oracle of tests/attention_oracle.py on inputs that make every single key visible: the census
(equal scores, an exact expectation, a tolerance of two output roundings), needles (one key
per probe at the chunk and partition edges), poisoned cache tails and unreferenced blocks,
and the staircase (a running max that grows on every tile).  tests/test_attention_oracle.py
shows on the CPU that each case fails for an oracle that drops, doubles, leaks or swaps ONE
token.  Every test prints its largest errors before it asserts."""
import pytest
import torch

import attention_oracle as ao
from kubernetes_gpu_cluster_amd import ops
from test_kernels_gpu import _DECODE_KERNELS, _use_decode_kernel

pytestmark = pytest.mark.gpu

KERNELS = list(_DECODE_KERNELS)


def _judge(what, case, got, exp, tol):
    bad, err, rel = ao.compare(got, exp, tol)
    print(f"\n[exact] {what} {ao.case_id(case)}: max abs err {err:.3e} max rel err {rel:.3e} "
          f"outside {bad}")
    assert bad == 0, f"{what}: {bad} elements outside {tol} (max abs {err:.3e}, rel {rel:.3e})"


def _decode(gpu, inp, exp, tol, what, case):
    q, kc, vc, bt, ctx = (t.to(gpu) for t in (inp.q, inp.kc, inp.vc, inp.bt, inp.ctx))
    for z in ao.DECODE_Z:
        out = torch.full_like(q, float("nan"))
        ops.paged_attention_decode(q, kc, vc, bt, ctx, inp.scale, grid_z=z, out=out,
                                   k_scale=inp.ks, v_scale=inp.vs)
        _judge(f"{what} z={z}", case, out, exp, tol)


@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("case", ao.DECODE_CENSUS_CASES, ids=ao.case_id)
def test_decode_census(gpu, monkeypatch, case, kern):
    """Every key weighs exactly 1 / ctx: contexts 1 .. 4097 across the 32-token chunk and
    64-token partition edges, z = 1, 3, 40, out pre-filled with NaN."""
    _use_decode_kernel(monkeypatch, kern)
    inp, exp, tol = ao.decode_census(*case)
    _decode(gpu, inp, exp, tol, f"decode census {kern}", case)


@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("case", ao.DECODE_NEEDLE_CASES, ids=ao.case_id)
def test_decode_needles(gpu, monkeypatch, case, kern):
    """Each (row, head) must find ITS key -- first tokens, chunk / partition edges, the last
    tokens -- through the score path, the mask and the online-softmax rescale."""
    _use_decode_kernel(monkeypatch, kern)
    inp, exp, tol = ao.decode_needles(*case)
    _decode(gpu, inp, exp, tol, f"decode needles {kern}", case)


@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("case", ao.FUSED_CASES, ids=ao.case_id)
def test_fused_decode_newest_token(gpu, monkeypatch, case, kern):
    """paged_attention_decode_rope: the newest token arrives through qkv and is written and
    read back inside the launch, over a stale decoy in its cache slot.  Judged by the float64
    oracle of the whole fused op; the cache changes in the written slots only."""
    _use_decode_kernel(monkeypatch, kern)
    inp, exp, tol = ao.fused_decode(*case)
    dev = {k: (v.to(gpu) if isinstance(v, torch.Tensor) else v) for k, v in vars(inp).items()
           if k != "state"}
    for z in ao.FUSED_Z:
        kc, vc = dev["kc"].clone(), dev["vc"].clone()
        out = ops.paged_attention_decode_rope(
            dev["qkv"], dev["pos"], dev["cs"], kc, vc, dev["slots"], inp.nq, inp.nkv, inp.d,
            dev["bt"], dev["ctx"], inp.scale, dev["qn"], dev["kn"], ao.EPS, grid_z=z,
            k_scale=inp.ks, v_scale=inp.vs, dtype=inp.dt)
        _judge(f"fused {kern} z={z}", case, out, exp, tol)
        # v is moved, not computed: the oracle's cache bytes; k within the value tolerance
        # (one e4m3 step where a last-bit difference crosses a rounding boundary); and
        # nothing but the written slots changes (the padding row writes nothing)
        assert torch.equal(vc.cpu().view(torch.uint8), inp.vc_after.view(torch.uint8))
        ktol = dict(atol=1e-3, rtol=0.13) if case[-1] else ao.value_tol(inp.dt, False)
        torch.testing.assert_close(kc.cpu().float(), inp.kc_after.float(), **ktol)
        bs = kc.shape[2]
        keep = torch.ones(kc.shape[0], bs, dtype=torch.bool)
        live = inp.slots[inp.slots >= 0]
        keep[live // bs, live % bs] = False
        assert torch.equal(kc.cpu().float().permute(0, 2, 1, 3)[keep],
                           inp.kc.float().permute(0, 2, 1, 3)[keep])


@pytest.mark.parametrize("persist", ["0", "1"])
@pytest.mark.parametrize("gqa", ["1", "0"])
@pytest.mark.parametrize("case", ao.PREFILL_CENSUS_CASES, ids=ao.case_id)
def test_prefill_census(gpu, monkeypatch, case, gqa, persist):
    """Every row of fresh prompts and chunked continuations (1 .. 2125 keys): the row at
    absolute position a counts keys 0 .. a exactly -- through prefill_attention and through
    prefill_attention_rope (q rotated as it is loaded; K = 0, so the census stands)."""
    monkeypatch.setenv("KGC_PREFILL_GQA", gqa)
    monkeypatch.setenv("KGC_PREFILL_PERSIST", persist)
    inp, exp, tol = ao.prefill_census(*case)
    q, qkv, kc, vc, bt, qsl, sl = (t.to(gpu) for t in (inp.q, inp.qkv, inp.kc, inp.vc, inp.bt,
                                                       inp.qsl, inp.sl))
    out = torch.full_like(q, float("nan"))
    ops.prefill_attention(q, kc, vc, bt, qsl, sl, inp.scale, out=out, k_scale=inp.ks,
                          v_scale=inp.vs)
    _judge(f"prefill census gqa={gqa} persist={persist}", case, out, exp, tol)
    from kubernetes_gpu_cluster_amd.ops import reference as ref
    cs = ref.rope_cos_sin_cache(inp.d, 4096, 5e5).to(gpu)
    out = torch.full_like(q, float("nan"))
    ops.prefill_attention_rope(qkv, cs, kc, vc, bt, qsl, sl, inp.scale, inp.nq, inp.d, out=out,
                               k_scale=inp.ks, v_scale=inp.vs)
    _judge(f"prefill-rope census gqa={gqa} persist={persist}", case, out, exp, tol)


@pytest.mark.parametrize("persist", ["0", "1"])
@pytest.mark.parametrize("gqa", ["1", "0"])
@pytest.mark.parametrize("case", ao.STAIRCASE_CASES, ids=ao.case_id)
def test_prefill_staircase(gpu, monkeypatch, case, gqa, persist):
    """The score rises by 2.0 / 2.83 per key: the row at position a lives on key a, a leaked
    key a + 1 or a lost key a is an O(1) error, and the running max grows on every tile."""
    monkeypatch.setenv("KGC_PREFILL_GQA", gqa)
    monkeypatch.setenv("KGC_PREFILL_PERSIST", persist)
    inp, exp, tol = ao.prefill_staircase(*case)
    q, kc, vc, bt, qsl, sl = (t.to(gpu) for t in (inp.q, inp.kc, inp.vc, inp.bt, inp.qsl, inp.sl))
    out = torch.full_like(q, float("nan"))
    ops.prefill_attention(q, kc, vc, bt, qsl, sl, inp.scale, out=out)
    _judge(f"prefill staircase gqa={gqa} persist={persist}", case, out, exp, tol)
