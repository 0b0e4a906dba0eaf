"""K16 (ops.logits_process, token_stats_init, token_stats_update) against a float64 per-row
reference: the ``_ref`` of tests/test_logits_processor.py in float64, min_p as probabilities.

Tolerance (derived): at most four fp32 operations, possibly contracted, carry a few 2^-24 of
relative error, which moves the rounding to the logits' dtype by at most one step: a touched
column equals the float64 result rounded to the dtype or a neighbour of it; 4 ulp for fp32.
Everything else comes back bit-identical.  Penalty parameters are exact in fp32.  A min_p
column within 1e-4 * t of the threshold could fall either way: the seeds are such that the
float64 reference finds none, and the reference side asserts that.
"""
import math

import numpy as np
import pytest
import torch

from kubernetes_gpu_cluster_amd import ops

NSLOTS, SENTINEL = 7, 768.0
# a row per rule alone, all four (the maximum only exists after the bias), an all -inf min_p row
SPECS = [dict(rep=1.25), dict(pres=-0.5, freq=0.25), dict(bias=True),
         dict(minp=0.3, t=0.75, plant=True),
         dict(rep=0.875, pres=-0.5, freq=0.125, bias=True, late_max=True, minp=0.05, t=1.0),
         dict(minp=0.2, t=1.0, allinf=True)]


def _bias(V, sp):
    # column 0, both sides of slice boundaries (chunks of 1024 / 8192), V - 1, >= V, a duplicate, -100
    e = [(0, 1.5), (V - 1, -2.0), (V + 3, 9.0), (5, 2.0), (3, -100.0), (5, 0.5)]
    e += [(c, v) for c, v in ((1023, 0.75), (1024, -1.25), (8191, 2.5), (8192, -0.75)) if c < V]
    return e + ([(V // 2, 30.0)] if sp.get("late_max") else [])


def _ref64(x, sp, prompt, output, V):
    """-> (expected float64 row, touched mask, smallest |distance to the min_p threshold|)"""
    x = x.clone()
    cnt = torch.zeros(V, dtype=torch.float64)
    for t in output:
        cnt[t] += 1
    seen = cnt > 0
    seen[prompt] = True
    touched = torch.zeros(V, dtype=torch.bool)
    if "rep" in sp or "freq" in sp:
        rep = sp.get("rep", 1.0)
        x = torch.where(seen & (x > 0), x / rep, torch.where(seen, x * rep, x))
        x = x - sp.get("freq", 0.0) * cnt - sp.get("pres", 0.0) * (cnt > 0).double()
        touched |= seen
    for i, v in (_bias(V, sp) if sp.get("bias") else []):
        if i < V:
            x[i] += v
            touched[i] = True
    margin = math.inf
    if sp.get("minp", 0) > 0:
        pr = torch.softmax(x / sp["t"], -1)
        keep = pr >= sp["minp"] * pr.max()
        fin = torch.isfinite(x)
        if fin.any():
            margin = (x[fin] - (x.max() + sp["t"] * math.log(sp["minp"]))).abs().min().item()
        x = torch.where(keep, x, torch.full_like(x, -math.inf))
        touched |= ~keep
    return x, touched, margin


def _ordinal(t):
    """Float bit patterns as integers that step by one per representable value."""
    bits = t.view(torch.int16 if t.element_size() == 2 else torch.int32).long()
    mag = bits & (0x7FFF if t.element_size() == 2 else 0x7FFFFFFF)
    return torch.where(bits < 0, -mag, mag)


def _run(dev, V, S, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + V)
    order = [4, 0, 2] if S == 5 else [0]
    groups = [SPECS[:3], SPECS[3:]] if S == 5 else [[s] for s in SPECS]
    slot_of = lambda r: (3 * r + 2) % NSLOTS                               # noqa: E731
    hi = min(V, 64)        # seen tokens sit in the first columns and at the very end
    prompts = {r: torch.randint(hi, (4,), generator=g).tolist() + [V - 1] for r in order}
    outputs = {r: torch.randint(hi, (6,), generator=g).tolist() + [V - 2, V - 2] for r in order}

    # statistics: the last token arrives through update; row 0's needs clamping, 4 and 2 repeat one
    stats = torch.full((NSLOTS, V), 12345, dtype=torch.int32, device=dev)
    want = np.full((NSLOTS, V), 12345, dtype=np.uint32)
    sampled = torch.zeros(S, dtype=torch.int64)
    for r in order:
        ops.token_stats_init(stats, slot_of(r), prompts[r], outputs[r][:-1])
        sampled[r] = V + 5 if r == 0 else outputs[r][-1]
    outputs[0][-1] = V - 1                       # what the clamp makes of V + 5
    table = ops.logits_table(order, [slot_of(r) for r in order], *[[0.0] * len(order)] * 5,
                             [[]] * len(order), dev)
    ops.token_stats_update(stats, table, sampled.to(dev))
    for r in order:
        w = np.zeros(V, dtype=np.uint32)
        w[prompts[r]] = 1 << 31
        np.add.at(w, outputs[r], 1)
        want[slot_of(r)] = w
    assert np.array_equal(stats.cpu().numpy().view(np.uint32), want)

    for contiguous in (True, False):
        for specs in groups:
            base = torch.full((S * (V + 11) + 1,), SENTINEL).to(dtype)
            view = base[1:].view(S, V + 11)[:, :V]                # odd element offset, padding
            view.copy_((torch.randn(S, V, generator=g) * 3).to(dtype))
            rows = order[:len(specs)]
            for r, sp in zip(rows, specs):
                view[r, prompts[r][0]] = view[r, outputs[r][0]] = -math.inf   # seen and -inf
                if sp.get("plant"):      # the maximum in the first slice, a survivor in the last
                    view[r, 1], view[r, V - 3] = 20.0, 19.5
                if sp.get("allinf"):
                    view[r] = -math.inf
            x = (view.contiguous() if contiguous else base.clone()).to(dev)
            uses = lambda sp: "rep" in sp or "freq" in sp                  # noqa: E731
            table = ops.logits_table(
                rows, [slot_of(r) if uses(sp) else -1 for r, sp in zip(rows, specs)],
                *[[sp.get(k, d) for sp in specs] for k, d in
                  (("pres", 0.0), ("freq", 0.0), ("rep", 1.0), ("minp", 0.0), ("t", 1.0))],
                [_bias(V, sp) if sp.get("bias") else [] for sp in specs], dev)
            for chunk in (0, 8192):
                full = x.clone()
                got = full if contiguous else full[1:].view(S, V + 11)[:, :V]
                ops.logits_process(got, stats, table, V, chunk=chunk)
                got = got.cpu()
                for r in range(S):
                    if r not in rows:
                        assert torch.equal(_ordinal(got[r]), _ordinal(view[r])), (r, "unprocessed")
                        continue
                    sp = specs[rows.index(r)]
                    exp, touched, margin = _ref64(view[r].double(), sp, prompts[r], outputs[r], V)
                    assert margin >= 1e-4 * sp.get("t", 1.0), ("min_p boundary: pick a seed", margin)
                    expd = exp.to(dtype)
                    d = (_ordinal(got[r]) - _ordinal(expd)).abs()
                    ok = (got[r] == expd) | (torch.isfinite(expd) & torch.isfinite(got[r])
                                             & (d <= (4 if dtype == torch.float32 else 1)))
                    ok &= touched | (_ordinal(got[r]) == _ordinal(view[r]))
                    assert bool(ok.all()), (r, sp, chunk, contiguous, (~ok).nonzero()[:8].tolist(),
                                            got[r][~ok][:8], expd[~ok][:8])
                if not contiguous:       # the padding and the element before the view
                    pad = full.cpu()
                    assert bool((pad[1:].view(S, V + 11)[:, V:] == SENTINEL).all()) and pad[0] == SENTINEL


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32],
                         ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("V", [8, 1000, 8192 + 5, 2 * 8192 + 3])
def test_logits_process_matches_float64(gpu, V, S, dtype):
    _run(gpu, V, S, dtype)


def test_reference_path_matches_float64():
    """The same judgement of ops/reference.py, which serves CPU tensors."""
    _run(torch.device("cpu"), 1000, 5, torch.float32)
