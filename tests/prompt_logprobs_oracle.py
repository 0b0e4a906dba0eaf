"""Float64 oracle of K15 prompt logprobs (numpy, CPU only; shares no code with
prompt_logprobs.hip or ops/reference.py), and the input matrix of its tests.

For a row of stored logits widened to float64 (exact for bf16 / f16 / fp32):

  lse      = M + log sum exp(x - M), M the row maximum
  token    x[target] - lse; -inf when the target's logit is -inf
  top-k    the k first columns in the order: value descending as floats (-0.0 == +0.0),
           equal values by ascending column id -- np.lexsort on (id, -value).  Fewer than
           k columns: the tail is (id -1, -inf).

Ids are judged exactly: selection works on stored values, which every dtype holds exactly.
Values are judged within BOUND(t, lse) = 1e-4 + 2^-20 max(|t|, |lse|): an fp32 sum of up to
2^18 terms taken as ~128 sequential adds per thread plus a ~20-level tree, hardware exp2 /
log2 at about 1 ulp, and the rounding of x * log2(e) for |x| <~ 90 come to about 2e-5;
1e-4 is the fp32-summation bound the sampler tests use (sampler_oracle.DELTA), and the
relative term covers the fp32 rounding of t - lse itself at large magnitudes.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import torch

import sampler_oracle as so

DELTA = 1e-4
REL = 2.0 ** -20


def bound(t, lse):
    t = np.where(np.isfinite(t), np.abs(t), 0.0)
    return DELTA + REL * np.maximum(t, np.abs(lse))


@dataclasses.dataclass
class Answer:
    lse: np.ndarray        # [R] float64
    tok: np.ndarray        # [R] float64 token logprob (-inf: target on a -inf column)
    tval: np.ndarray       # [R] float64 the target's stored logit
    ids: np.ndarray        # [R, K] int64, -1 padded
    vals: np.ndarray       # [R, K] float64 stored logits of ids (-inf padded)


def oracle(x, targets, k: int, col0: int = 0) -> Answer:
    """x: [R, V] array-like of stored logits; targets: [R] global ids (col0 = id of column 0)."""
    x = np.asarray(x, dtype=np.float64)
    R, V = x.shape
    lse, tok, tval = np.empty(R), np.empty(R), np.empty(R)
    ids = np.full((R, k), -1, dtype=np.int64)
    vals = np.full((R, k), -np.inf)
    for r in range(R):
        row = x[r]
        M = row.max() if V else -np.inf
        lse[r] = M + np.log(np.exp(row - M).sum()) if np.isfinite(M) else -np.inf
        t = int(targets[r]) - col0
        tval[r] = row[t] if 0 <= t < V else -np.inf
        tok[r] = tval[r] - lse[r] if np.isfinite(tval[r]) else -np.inf
        if k:
            order = np.lexsort((np.arange(V), -(row + 0.0)))[:k]     # + 0.0: -0.0 -> +0.0
            ids[r, :order.size] = order + col0
            vals[r, :order.size] = row[order]
    return Answer(lse, tok, tval, ids, vals)


def check(ans: Answer, k: int, tok, top_lp, top_id, what: str = "") -> tuple:
    """Every row: ids exact, values within bound().  Returns (the largest error, the
    largest error as a share of its bound)."""
    tok = np.asarray(tok, dtype=np.float64)
    top_lp = np.asarray(top_lp, dtype=np.float64).reshape(tok.size, k)
    top_id = np.asarray(top_id, dtype=np.int64).reshape(tok.size, k)
    assert not np.isnan(tok).any() and not np.isnan(top_lp).any(), f"{what}: NaN"
    want_id = ans.ids[:, :k]
    assert (top_id == want_id).all(), \
        f"{what}: ids differ in rows {np.flatnonzero((top_id != want_id).any(1))[:8].tolist()}"
    worst, share = 0.0, 0.0
    inf_t = ~np.isfinite(ans.tok)
    assert (tok[inf_t] == -np.inf).all(), f"{what}: -inf target rows {tok[inf_t][:4]}"
    err = np.abs(tok[~inf_t] - ans.tok[~inf_t])
    b = bound(ans.tval[~inf_t], ans.lse[~inf_t])
    assert (err <= b).all(), f"{what}: token logprob error {err.max()} (bound {b.min()})"
    if err.size:
        worst, share = float(err.max()), float((err / b).max())
    want = ans.vals[:, :k] - ans.lse[:, None]
    inf_v = ~np.isfinite(ans.vals[:, :k])
    assert (top_lp[inf_v] == -np.inf).all(), f"{what}: -inf candidates"
    err = np.abs(np.where(inf_v, 0.0, top_lp - np.where(inf_v, 0.0, want)))
    b = bound(np.where(inf_v, 0.0, ans.vals[:, :k]), np.broadcast_to(ans.lse[:, None], want.shape))
    assert (err <= b).all(), f"{what}: top logprob error {err.max()}"
    if err.size:
        worst, share = max(worst, float(err.max())), max(share, float((err / b).max()))
    return worst, share


# ------------------------------------------------------------------ the test matrix
DTYPES = so.DTYPES
KS = (0, 1, 5, 20)
KMAX = 20
FAMILIES = ("gauss1", "gauss10", "peaked", "flat", "quant", "masked1", "tgtinf", "szero", "huge")
SHAPES = [(R, V) for R in (1, 3, 17) for V in (8, 1000, 4104, 50257)] + [(1, 128256)]
LAYOUT_SHAPES = [(3, 1000), (3, 50257)]


def _row(fam: str, V: int, dt: torch.dtype, gen: torch.Generator):
    """(fp32 row, target or None)."""
    if fam == "gauss10":
        return so.family_row("gauss1", V, gen) * 10.0, None
    if fam in ("gauss1", "peaked", "flat", "quant", "masked1"):
        return so.family_row(fam, V, gen), None
    if fam == "tgtinf":                    # the target sits on a -inf column
        row = so.family_row("masked7", V, gen)
        dead = torch.nonzero(torch.isinf(row)).flatten()
        return row, int(dead[int(torch.randint(len(dead), (1,), generator=gen))])
    if fam == "szero":                     # 2 positives, then +-0.0: the k boundary is in the zeros
        row = -(torch.randn(V, generator=gen).abs() * 3 + 1)
        p = torch.randperm(V, generator=gen)
        nz = min(max(V // 2, 3), 40)
        z = p[2:2 + nz]
        row[p[:2]] = torch.tensor([2.0, 1.0])
        row[z] = 0.0
        row[z[torch.rand(nz, generator=gen) < 0.5]] = -0.0
        return row, int(z[0])
    if fam == "huge":                      # magnitudes near the dtype's maximum
        top = 6.0e4 if dt == torch.float16 else 1.0e38
        row = torch.where(torch.rand(V, generator=gen) < 0.5, top, -top) * \
            (1.0 - 0.01 * torch.rand(V, generator=gen))
        return row, None
    raise KeyError(fam)


@dataclasses.dataclass
class Case:
    name: str
    dtype: torch.dtype
    layout: str              # contig | wide | offset (as sampler_oracle.Case)
    logits: torch.Tensor     # [R, V] stored dtype, CPU
    targets: torch.Tensor    # [R] int64

    def place(self, device) -> torch.Tensor:
        """The logits on `device` in the case's layout; columns outside the view hold +60."""
        R, V = self.logits.shape
        if self.layout == "contig":
            return self.logits.to(device)
        big = torch.full((R, V + 24), 60.0, dtype=self.dtype, device=device)
        view = big[:, :V] if self.layout == "wide" else big[:, 3:3 + V]
        view.copy_(self.logits)
        return view

    def shards(self, n: int, device):
        """TP-style column shards: n of ceil(V / n) columns (the last ones part or all
        padding, which holds +60), plus one shard of padding only (ncols = 0).
        -> [(tensor [R, per], vocab_off, ncols)]."""
        R, V = self.logits.shape
        per = -(-V // n)
        out = []
        for i in range(n + 1):
            off = min(i * per, V)
            nc = max(0, min(per, V - i * per))
            t = torch.full((R, per), 60.0, dtype=self.dtype, device=device)
            t[:, :nc] = self.logits[:, off:off + nc]
            out.append((t, off, nc))
        return out


def make_case(name: str, dtype_name: str, R: int, V: int, layout: str, start: int) -> Case:
    dt = DTYPES[dtype_name]
    gen = torch.Generator().manual_seed(7919 * start + 31 * V + R)
    rows, tg = [], []
    for r in range(R):
        fam = FAMILIES[(start + r) % len(FAMILIES)]
        row, t = _row(fam, V, dt, gen)
        if t is None:
            t = (0, V - 1)[r % 2] if (start + r) % 5 == 0 else int(torch.randint(V, (1,), generator=gen))
        rows.append(row.to(dt))
        tg.append(t)
    return Case(name, dt, layout, torch.stack(rows), torch.tensor(tg, dtype=torch.int64))


def case_specs() -> list[tuple]:
    specs, start = [], 0
    for R, V in SHAPES:
        for dn in DTYPES:
            specs.append((f"{dn}-R{R}-V{V}", dn, R, V, "contig", start))
            start += R + 2
    for R, V in LAYOUT_SHAPES:
        for dn in DTYPES:
            for layout in ("wide", "offset"):
                specs.append((f"{dn}-R{R}-V{V}-{layout}", dn, R, V, layout, start))
                start += R + 2
    return specs


CASE_NAMES = [s[0] for s in case_specs()]


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    return make_case(*next(s for s in case_specs() if s[0] == name))


@functools.lru_cache(maxsize=None)
def answer(name: str) -> Answer:
    """The oracle's answer at k = KMAX, computed once; a smaller k is its prefix."""
    c = case(name)
    return oracle(c.logits.double().numpy(), c.targets.numpy(), KMAX)
