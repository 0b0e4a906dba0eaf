"""The float64 sampler oracle (tests/sampler_oracle.py) on the CPU: hand-made rows with known
answers, agreement with ops.reference.sample on every sharp row of the GPU edge matrix, and
the cap on banded rows that keeps the tolerance band from hiding failures."""
import numpy as np
import pytest
import torch

import sampler_oracle as so
from kubernetes_gpu_cluster_amd.ops import reference as ref


def _row(vals, t=1.0, k=-1, p=1.0, seed=3, delta=None):
    r = np.asarray(vals, dtype=np.float64)
    g = so.noise(torch.tensor([seed]), r.size)[0]
    return so.judge_row(r, t, k, p, g, delta), r / max(t, 1e-30) + g


def test_ulp32():
    assert so.ulp32(1.0) == 2.0 ** -23
    assert so.ulp32(1.999) == 2.0 ** -23
    assert so.ulp32(-2.0) == 2.0 ** -22
    assert so.ulp32(3.0e4) == 2.0 ** -9
    assert so.ulp32(0.0) == 2.0 ** -149


def test_greedy_is_first_index_of_the_maximum():
    for t in (0.0, float(np.float32(1e-5))):
        v, _ = _row([1.0, 7.0, -3.0, 7.0, 2.0], t=t, k=1, p=0.5)
        assert v.greedy and v.sharp and v.accept.tolist() == [1]
    v, _ = _row([1.0, 7.0, -3.0, 7.0, 2.0], t=float(np.float32(2e-5)))
    assert not v.greedy


def test_top_k_keeps_ties_and_compares_exactly():
    vals = [5.0, 1.0, 3.0, 3.0, 3.0 - 2.0 ** -20, 0.0, 9.0, 3.0]
    for seed in range(40):
        v, s = _row(vals, k=3, seed=seed)
        assert v.threshold and v.n_lo == v.n_hi == 5           # 9, 5 and the three 3.0
        sup = [0, 2, 3, 6, 7]
        assert v.accept.tolist() == [sup[int(np.argmax(s[sup]))]]
    for k in (0, -1, 8, 13):                                   # disabled forms
        v, s = _row(vals, k=k)
        assert not v.threshold and v.n_hi == 8 and v.accept.tolist() == [int(np.argmax(s))]


def test_top_k_signed_zeros_are_one_tie_group():
    vals = [2.0, 0.0, -0.0, 1.0, -0.0, 0.0, -1.0, -5.0]
    v, _ = _row(vals, k=3)                                     # the 3rd largest is a zero
    assert v.n_hi == 6
    v, _ = _row(vals, k=3, p=0.9)
    # the masses above the zeros are e^2 + e = 10.11 of z = 14.11: 0.9 z falls into the zeros
    assert v.n_lo == v.n_hi == 6


def test_nucleus_rule_and_band():
    # masses 0.5, 0.25, 0.125, 0.125 (a tie group)
    vals = np.log([0.5, 0.25, 0.125, 0.125])
    assert _row(vals, p=0.4)[0].n_hi == 1
    assert _row(vals, p=0.6)[0].n_hi == 2
    assert _row(vals, p=0.76)[0].n_hi == 4                     # 0.75 < p: the whole tie group
    assert _row(vals, p=1e-6)[0].n_hi == 1
    # p on a boundary: "mass before < p" is decided by rounding -> the band spans it
    v, _ = _row(vals, p=0.75)
    assert (v.n_lo, v.n_hi) == (2, 4)
    v, _ = _row(vals, p=0.75 * (1 + 2e-4))
    assert (v.n_lo, v.n_hi) == (4, 4)
    # temperature reshapes the masses: t = 0.5 squares them -> 16, 4, 1, 1 of 22
    assert _row(vals, t=0.5, p=0.7)[0].n_hi == 1
    assert _row(vals, t=0.5, p=0.75)[0].n_hi == 2
    # top-p acts on the top-k support: k = 2 leaves 2/3, 1/3
    assert _row(vals, k=2, p=0.6)[0].n_hi == 1
    assert _row(vals, k=2, p=0.7)[0].n_hi == 2


def test_masked_rows_and_undefined_rows():
    ninf = float("-inf")
    v, s = _row([ninf, 1.0, ninf, ninf, 0.5, ninf], k=4, p=0.99)    # the 4th largest is -inf
    assert v.ok(int(np.argmax(s))) and set(v.accept.tolist()) <= {1, 4}
    v, _ = _row([ninf, 1.0, ninf, ninf], t=100.0)
    assert v.accept.tolist() == [1]
    for bad in ([ninf] * 4, [1.0, float("nan")], [1.0, float("inf")]):
        with pytest.raises(ValueError):
            _row(bad)


def test_score_slack_makes_near_ties_banded():
    # two tokens whose scores differ by less than 4 ulp32(|r / t|): either may win
    g = so.noise(torch.tensor([5]), 2)[0]
    t = 1e-4
    r = np.array([3.0, 3.0 + (g[0] - g[1]) * t])              # s0 == s1 up to rounding
    v = so.judge_row(r, t, -1, 1.0, g)
    assert v.accept.tolist() == [0, 1] and not v.sharp
    r[1] -= 16 * so.ulp32(3.0 / t) * t
    assert so.judge_row(r, t, -1, 1.0, g).accept.tolist() == [0]


@pytest.mark.parametrize("name", so.CASE_NAMES)
def test_oracle_agrees_with_reference_on_sharp_rows(name):
    c = so.case(name)
    vs = so.case_verdicts(name)
    exp = ref.sample(c.logits, c.temperature, c.top_k, c.top_p, c.seeds).tolist()
    bad = [(b, c.families[b], exp[b], v.accept.tolist()) for b, v in enumerate(vs)
           if v.sharp and not v.ok(exp[b])]
    assert not bad, bad[:8]
    # and on banded rows the reference's token is one the oracle accepts
    assert all(v.ok(exp[b]) for b, v in enumerate(vs))


def test_banded_share_is_capped():
    """The band must not hide failures: per case at most a quarter of the threshold rows
    are banded, over the matrix at most a tenth."""
    tot = banded = 0
    worst = []
    for name in so.CASE_NAMES:
        thr = [v for v in so.case_verdicts(name) if v.threshold]
        nb = sum(not v.sharp for v in thr)
        tot += len(thr)
        banded += nb
        if 4 * nb > len(thr):
            worst.append((name, nb, len(thr)))
    print(f"banded threshold rows: {banded} of {tot}")
    assert not worst, worst
    assert tot > 2000 and 10 * banded <= tot


def test_matrix_covers_every_family_kind_and_temperature():
    seen_fk, seen_ft = set(), set()
    for name in so.CASE_NAMES:
        c = so.case(name)
        V = c.logits.shape[1]
        for b, fam in enumerate(c.families):
            k, p = int(c.top_k[b]), float(c.top_p[b])
            kind = ("k" if 0 < k < V else "") + ("p" if p < 1 else "")
            seen_fk.add((fam, kind))
            seen_ft.add((fam, round(float(c.temperature[b]), 6)))
    fams = [f for f in so.FAMILIES if f != "szero"]            # szero: always k with p
    assert all((f, kind) in seen_fk for f in fams for kind in ("kp", "k", "p", ""))
    assert ("szero", "kp") in seen_fk
    assert all((f, round(float(np.float32(t)), 6)) in seen_ft for f in fams for t in so.TEMPS)
