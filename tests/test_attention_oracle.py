"""The float64 attention oracle (tests/attention_oracle.py) checked on the CPU: it agrees with
ops.reference on random inputs, every builder's conditions hold on exactly the cases
tests/test_attention_exact_gpu.py runs, the unmutated oracle -- rounded to the output dtype --
passes each case's comparison, and every mutant of the key list FAILS it."""
import numpy as np
import pytest
import torch

import attention_oracle as ao
from kubernetes_gpu_cluster_amd.ops import reference as ref

# Mutants that are mathematically invisible, by name: the oracle's answer does not change
# (or changes by less than one part in 1e6), so no comparison can see them.
#   census / swap_v      the census is a sum over tokens: trading the V of two attended
#                        tokens changes nothing.
#   census / dup_last    at a context of ONE token (the same key twice is the same softmax);
#                        every census case has longer rows, so the case still fails.
#   census / drop_chunk  rows of <= 32 tokens have no key in [32, 64); longer rows do.
#   needles / dup_last   the doubled key is either the needle (its weight stays ~1) or
#                        filler (weight ~1e-9): the census carries this mutant.
INVISIBLE = {
    "census": {"swap_v"},
    "needle": {"dup_last"},
    "staircase": set(),
}


def _passes(exp, dt, tol, ref_exp):
    return ao.compare(ao.rounded(exp, dt), ref_exp, tol)[0] == 0


def _rand_cache(ctx, nkv, bs, d, dt, seed):
    g = torch.Generator().manual_seed(seed)
    need = [(c + bs - 1) // bs for c in ctx]
    nb = sum(need) + 3
    kc = (torch.randn(nb, nkv, bs, d, generator=g) * 0.5).to(dt)
    vc = torch.randn(nb, nkv, bs // 8, d, 8, generator=g).to(dt)
    perm = torch.randperm(nb, generator=g).tolist()
    bt = torch.zeros(len(ctx), max(need) + 1, dtype=torch.int32)
    at = 0
    for b, n in enumerate(need):
        bt[b, :n] = torch.tensor(perm[at:at + n], dtype=torch.int32)
        at += n
    return kc, vc, bt, g


@pytest.mark.parametrize("fp8", [False, True])
def test_oracle_matches_reference_decode(fp8):
    ctx, nq, nkv, d, bs = [1, 17, 64, 129], 8, 2, 64, 16
    kc, vc, bt, g = _rand_cache(ctx, nkv, bs, d, torch.float32, 1)
    ks, vs = (0.5, 0.25) if fp8 else (1.0, 1.0)
    if fp8:
        kc, vc = ref.to_cache(kc, ao.FP8, ks), ref.to_cache(vc, ao.FP8, vs)
    q = torch.randn(len(ctx), nq, d, generator=g)
    exp = ref.paged_attention_decode(q, kc, vc, bt, torch.tensor(ctx), d ** -0.5, ks, vs)
    got = ao.decode(ao.widen(q), ao.paged_kv(kc, vc, bt, ks, vs), ctx, d ** -0.5)
    np.testing.assert_allclose(got, exp.double().numpy(), atol=2e-6, rtol=1e-5)
    # ... and attend on one row, one head, by hand
    k, v = ao.kv_positions(kc, vc, bt[3], ks, vs)
    one = ao.attend(ao.widen(q)[3, 5], k[:, 1], v[:, 1], d ** -0.5, list(range(129)))
    np.testing.assert_allclose(one, got[3, 5], atol=1e-14)


def test_oracle_matches_reference_prefill():
    seq, query, nq, nkv, d, bs = [5, 70, 131], [5, 20, 131], 4, 2, 64, 16
    kc, vc, bt, g = _rand_cache(seq, nkv, bs, d, torch.float32, 2)
    q = torch.randn(sum(query), nq, d, generator=g)
    qsl = torch.tensor([0, 5, 25, 156])
    exp = ref.prefill_attention(q, kc, vc, bt, qsl, torch.tensor(seq), d ** -0.5)
    got = ao.prefill(ao.widen(q), kc, vc, bt, query, seq, d ** -0.5)
    np.testing.assert_allclose(got, exp.double().numpy(), atol=2e-6, rtol=1e-5)


@pytest.mark.parametrize("qk_norm", [False, True])
@pytest.mark.parametrize("S", [0, 3])
def test_oracle_matches_reference_rope_write(qk_norm, S):
    B, nq, nkv, d, bs, nb = 9, 4, 2, 64, 16, 6
    g = torch.Generator().manual_seed(3)
    N = (nq + 2 * nkv) * d
    qkv = torch.randn(*((S, B, N) if S else (B, N)), generator=g)
    pos = torch.randint(0, 500, (B,), generator=g)
    slots = torch.randperm(nb * bs, generator=g)[:B]
    slots[4] = -1
    cs = ref.rope_cos_sin_cache(d, 512, 5e5)
    qn = torch.randn(d, generator=g) if qk_norm else None
    kn = torch.randn(d, generator=g) if qk_norm else None
    kc, vc = torch.zeros(nb, nkv, bs, d), torch.zeros(nb, nkv, bs // 8, d, 8)
    kc2, vc2 = kc.clone(), vc.clone()
    q = ao.fused_write(qkv, pos, cs, kc, vc, slots, nq, nkv, d, qn, kn, 1e-6, torch.float32)
    summed = qkv.double().sum(0).float() if S else qkv
    qr = ref.rope_qk_kv_write(summed, pos, cs, kc2, vc2, slots, nq, nkv, d, qn, kn, 1e-6)
    np.testing.assert_allclose(q, qr.double().numpy(), atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(kc, kc2, atol=1e-5, rtol=1e-5)
    assert torch.equal(vc, vc2)


def test_census_analytic_equals_attend():
    """The analytic census expectation is what the oracle computes from the stored cache,
    for the clean key list and for a mutant's."""
    for case in (ao.DECODE_CENSUS_CASES[0], ao.DECODE_CENSUS_CASES[-1]):
        inp, exp, _ = ao.decode_census(*case)
        kv = ao.decode_kv(inp)
        np.testing.assert_allclose(ao.decode_expected(inp, None, kv), exp, atol=1e-13)
        np.testing.assert_allclose(ao.decode_expected(inp, "drop_chunk", kv),
                                   ao.decode_census_expected(inp, "drop_chunk"), atol=1e-13)
    # prefill: the first four sequences (a leak past the 5-token one lands on the poisoned
    # tail of its block, past the 64-token one on block 0 through the unused table entry)
    inp, exp, _ = ao.prefill_census(*ao.PREFILL_CENSUS_CASES[3])
    T = sum(inp.query[:4])
    for m in (None, "dup_last", "drop_chunk", ao.LEAK):
        got = ao.prefill(ao.widen(inp.q)[:T], inp.kc, inp.vc, inp.bt[:4], inp.query[:4],
                         inp.seq[:4], inp.scale, inp.ks, inp.vs, m)
        np.testing.assert_allclose(got, ao.prefill_census_expected(inp, m)[:T], atol=1e-12)


def test_census_resolves_one_token():
    """The condition behind the census tolerance, at the sizes where it is tightest: with
    at most 64 positions per class, one token more or less moves some channel by 1 / 64 of
    itself (less the 1 / ctx by which every channel moves): 4x the bf16 tolerance."""
    for d, ctx in ((128, 2049), (128, 8192), (64, 4096), (128, 129)):
        base = ao.census_expected(np.arange(ctx), 0, d, 1.0)
        for keys in (np.arange(ctx - 1), np.arange(1, ctx), np.r_[np.arange(ctx), ctx - 1],
                     np.delete(np.arange(ctx), ctx // 2)):
            mut = ao.census_expected(keys, 0, d, 1.0)
            nz = base > 0
            assert (np.abs(mut - base)[nz] / base[nz]).max() >= 2.0 ** -6 * (1 - 65 / ctx)
            for dt in ao.DTYPES:
                tol = ao.census_tol(dt)
                assert ao.compare(ao.rounded(mut, dt), base, tol)[0] > 0
                assert ao.compare(ao.rounded(base, dt), base, tol)[0] == 0


def _judge(kind, dt, tol, exp, mutants):
    """The clean oracle passes; every mutant fails -- but the ones named invisible, which
    are shown to be just that."""
    assert _passes(exp, dt, tol, exp), "the clean oracle, rounded, must pass"
    for name, make in mutants.items():
        assert _passes(make(), dt, tol, exp) == (name in INVISIBLE[kind]), f"mutant {name}"


@pytest.mark.parametrize("case", ao.DECODE_CENSUS_CASES, ids=ao.case_id)
def test_decode_census_mutants(case):
    inp, exp, tol = ao.decode_census(*case)
    assert tol == ao.census_tol(case[0])
    _judge("census", case[0], tol, exp,
           {m: (lambda m=m: ao.decode_census_expected(inp, m)) for m in ao.MUTANTS
            if m != "swap_v"})
    # the invisible ones of single rows, stated: ctx 1 doubled, no chunk [32, 64) below 33
    ctx = inp.ctx.tolist()
    dup, chunk = (ao.decode_census_expected(inp, m) for m in ("dup_last", "drop_chunk"))
    for b, c in enumerate(ctx):
        assert np.array_equal(dup[b], exp[b]) == (c == 1)
        assert np.array_equal(chunk[b], exp[b]) == (c <= 32)


@pytest.mark.parametrize("case", ao.DECODE_NEEDLE_CASES, ids=ao.case_id)
def test_decode_needle_mutants(case):
    inp, exp, tol = ao.decode_needles(*case)       # asserts the needle weights
    kv = ao.decode_kv(inp)
    _judge("needle", case[0], tol, exp,
           {m: (lambda m=m: ao.decode_expected(inp, m, kv)) for m in ao.MUTANTS})


@pytest.mark.parametrize("case", ao.FUSED_CASES, ids=ao.case_id)
def test_fused_decode_mutants(case):
    kind, dt = case[0], case[1]
    inp, exp, tol = ao.fused_decode(*case)
    stale = ao.fused_state(inp, write=False)
    mutants = {m: (lambda m=m: ao.fused_expected(inp, m, state=inp.state)) for m in ao.MUTANTS}
    mutants[ao.STALE] = lambda: ao.fused_expected(inp, ao.STALE, state=stale)
    _judge(kind, dt, tol, exp, mutants)
    assert np.all(exp[-1] == 0)                     # the padding row


@pytest.mark.parametrize("case", ao.PREFILL_CENSUS_CASES, ids=ao.case_id)
def test_prefill_census_mutants(case):
    inp, exp, tol = ao.prefill_census(*case)
    _judge("census", case[0], tol, exp,
           {m: (lambda m=m: ao.prefill_census_expected(inp, m))
            for m in ao.MUTANTS + (ao.LEAK,) if m != "swap_v"})


@pytest.mark.parametrize("case", ao.STAIRCASE_CASES, ids=ao.case_id)
def test_prefill_staircase_mutants(case):
    inp, exp, tol = ao.prefill_staircase(*case)    # asserts the excluded mass
    # the window is the whole answer: the first rows past it, summed over every key
    q = ao.widen(inp.q)
    lo = 64 + ao.WINDOW
    full = ao.prefill(q[lo:lo + 8], inp.kc, inp.vc, inp.bt[:1], [8], [lo + 8], inp.scale)
    np.testing.assert_allclose(full, exp[lo:lo + 8], atol=1e-11)
    # the row at position a puts 0.86 (d = 64) / 0.94 (d = 128) of its mass on key a
    step = inp.scale * (32.0 if inp.d == 128 else 16.0)
    assert abs((1 - np.exp(-step)) - (0.94 if inp.d == 128 else 0.86)) < 0.01
    _judge("staircase", case[0], tol, exp,
           {m: (lambda m=m: ao.prefill_expected(inp, m, ao.WINDOW))
            for m in ao.MUTANTS + (ao.LEAK,)})
