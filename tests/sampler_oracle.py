"""Float64 oracle of the K10 sampler (CPU only; shares no code with sampling.hip).

For one row -- the stored logits widened to float64 (exact for bf16 / f16 / fp32), the
fp32 temperature and top-p, top-k and the seed -- ``judge_row`` computes the set of token
ids a correct sampler may return:

  noise    g_i = ref.gumbel(ref.uniform_noise(seed, V)), widened to float64: these two
           define the generator.
  score    s_i = r_i / t + g_i in float64.
  top-k    r_i >= the k-th largest stored value, ties kept.  Stored values compare
           exactly: no tolerance.  (-0.0 == +0.0, as in every float comparison.)
  top-p    float64 softmax over that support, and the nucleus by ref.sample's rule: a
           token is kept iff the mass of the strictly larger values is < p (whole tie
           groups).  Evaluated at p (1 - DELTA) and at min(p (1 + DELTA), 1): N_lo within
           N_hi.
  accept   got is in N_hi, and s[got] >= max(s over N_lo) - 4 ulp32(|r / t|), the ulp
           taken at the larger |r / t| of the two tokens compared.
  greedy   t <= 1e-5: exactly the first index of the maximum.

A row whose accepted set is ONE token is *sharp* (the sampler must return exactly that
token); every other row is *banded*.  That covers the rows with N_lo == N_hi whose best
score clears the runner-up by more than the slack, and also the rows where N_hi is larger
but none of its extra tokens comes within the slack of the best score of N_lo: there too
one token is right, and the tests hold the kernel to it.

DELTA = 1e-4 relative.  The kernel forms p * z and the running mass in fp32 from up to
2^17 positive terms, summed hierarchically (per thread, per workgroup, then atomics): a
random-walk error of about sqrt(n) * 2^-24 = 2e-5; __expf carries the rounding of an
argument of up to ~32 nats, about 3e-6.  1e-4 is about five times their sum.
SLACK_ULP = 4.  The kernel forms r * (1 / t) + g in fp32 (possibly one FMA), the oracle
r / t + g: at most about 2 ulp of |r / t| per token, for two tokens.

``cases()`` builds the inputs of tests/test_sampler_edges_gpu.py; tests/test_sampler_oracle.py
checks the oracle and the share of banded rows on exactly those inputs.
"""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np
import torch

from kubernetes_gpu_cluster_amd.ops import reference as ref

DELTA = 1e-4
SLACK_ULP = 4.0
_GREEDY = float(np.float32(1e-5))


def ulp32(x):
    """The fp32 unit in the last place at |x| (float64 array in, float64 out)."""
    a = np.abs(np.asarray(x, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -126)))
    return np.exp2(np.minimum(e, 127.0) - 23.0)


@dataclasses.dataclass
class Verdict:
    accept: np.ndarray      # sorted token ids a correct sampler may return
    greedy: bool
    threshold: bool         # the row uses top-k or top-p
    n_lo: int               # |N_lo|, |N_hi| (both the support size without top-p)
    n_hi: int

    @property
    def sharp(self) -> bool:
        return self.accept.size == 1

    def ok(self, got: int) -> bool:
        i = int(np.searchsorted(self.accept, got))
        return i < self.accept.size and int(self.accept[i]) == int(got)


def _nucleus(r, sup, t, p_lo, p_hi):
    """Masks of N_lo and N_hi: the tokens of `sup` whose strictly-larger mass is < p * Z."""
    rs = r[sup]
    w = np.exp((rs - rs.max()) / t)                         # -inf -> 0
    vals, inv = np.unique(rs, return_inverse=True)          # ascending; -0.0 == +0.0
    gm = np.bincount(inv.reshape(-1), weights=w, minlength=vals.size)
    incl = np.cumsum(gm[::-1])[::-1]                        # mass of values >= this one
    above = incl - gm
    z = incl[0]
    out = []
    for pp in (p_lo, p_hi):
        m = np.zeros(r.size, dtype=bool)
        m[sup] = (above < pp * z)[inv.reshape(-1)]
        out.append(m)
    return out


def judge_row(r, t, k, p, g, delta=None) -> Verdict:
    """r: float64 [V] stored logits; t, p: the fp32 values as Python floats; k: int;
    g: float64 [V] Gumbel noise of the row's seed."""
    delta = DELTA if delta is None else delta
    r = np.asarray(r, dtype=np.float64)
    V = r.size
    if np.isnan(r).any() or not np.isfinite(r).any() or np.isposinf(r).any():
        raise ValueError("row has no defined answer (NaN, +inf, or all -inf)")
    if t <= _GREEDY:
        return Verdict(np.array([int(np.argmax(r))]), True, False, V, V)
    use_k, use_p = 0 < k < V, p < 1.0
    if use_p and not p > 0.0:
        raise ValueError("top_p <= 0 has no defined answer")
    sup = np.ones(V, dtype=bool)
    if use_k:
        sup = r >= np.partition(r, V - k)[V - k]
    lo = hi = sup
    if use_p:
        lo, hi = _nucleus(r, sup, t, p * (1.0 - delta), min(p * (1.0 + delta), 1.0))
    x = r / t
    s = x + g
    best = int(np.argmax(np.where(lo, s, -np.inf)))
    cand = np.flatnonzero(hi & np.isfinite(s))
    slack = SLACK_ULP * ulp32(np.maximum(np.abs(x[cand]), abs(x[best])))
    acc = cand[s[cand] >= s[best] - slack]
    return Verdict(acc, False, use_k or use_p, int(lo.sum()), int(hi.sum()))


def noise(seeds: torch.Tensor, V: int, col0: int = 0) -> np.ndarray:
    """float64 [B, V]: the Gumbel noise of the global columns col0 .. col0 + V - 1."""
    return ref.gumbel(ref.uniform_noise_cols(seeds.cpu(), col0, V)).double().numpy()


def judge(logits, temperature, top_k, top_p, seeds, delta=None) -> list[Verdict]:
    """Verdicts for every row of a batch (tensors as ops.sample takes them, any device)."""
    x = logits.detach().cpu().double().numpy()
    t = temperature.detach().cpu().float().double().tolist()
    k = top_k.detach().cpu().tolist()
    p = top_p.detach().cpu().float().double().tolist()
    B, V = x.shape
    out = []
    for b0 in range(0, B, 32):                       # noise in slabs: bounded memory
        g = noise(seeds[b0:b0 + 32], V)
        out += [judge_row(x[b], t[b], int(k[b]), p[b], g[b - b0], delta)
                for b in range(b0, min(B, b0 + 32))]
    return out


def check(got, verdicts, what="") -> None:
    """Every row's sampled id is one its verdict accepts (sharp rows: the one token)."""
    got = [int(v) for v in got.detach().cpu().tolist()]
    bad = [(b, got[b], "sharp" if v.sharp else "banded", v.accept[:4].tolist(), v.n_lo, v.n_hi)
           for b, v in enumerate(verdicts) if not v.ok(got[b])]
    assert not bad, f"{what}: {len(bad)} of {len(got)} rows rejected " \
                    f"(row, got, kind, accepted, |N_lo|, |N_hi|): {bad[:8]}"


# ------------------------------------------------------------------ the test matrix
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "fp32": torch.float32}
FAMILIES = ("gauss1", "gauss3", "gauss8", "peaked", "masked1", "masked2", "masked7", "masked60",
            "flat", "quant", "zipf", "szero")
_P_BELOW_1 = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
# (top_k, top_p); top_k "V-1", "V", "V+5" are resolved per vocabulary
KINDS = ((50, 0.9), (5, 0.5), (2, 0.99),                    # top-k with top-p
         (1, 1.0), (2, 1.0), ("V-1", 1.0),                  # top-k alone
         ("V", 1.0), ("V+5", 1.0), (-1, 1.0),               # disabled forms of top-k
         (-1, 1e-6), (-1, 0.1), (-1, 0.95), (-1, _P_BELOW_1))   # top-p alone
TEMPS = (0.0, 1e-5, 2e-5, 1e-4, 0.3, 0.7, 1.0, 1.3, 100.0)
SEEDS = (-1, 0, 2 ** 63 - 1, -2 ** 63, (5 << 32) + 17, 2 ** 40 + 3, 123456789, (1 << 33) - 1)


def family_row(fam: str, V: int, gen: torch.Generator) -> torch.Tensor:
    """One fp32 row of the family (rounded to the stored dtype by the caller)."""
    n = torch.randn(V, generator=gen)
    if fam.startswith("gauss"):
        return n * float(fam[5:])
    if fam == "peaked":
        n[int(torch.randint(V, (1,), generator=gen))] += 20.0
        return n
    if fam.startswith("masked"):
        keep = torch.randperm(V, generator=gen)[:min(int(fam[6:]), V)]
        row = torch.full((V,), float("-inf"))
        row[keep] = n[keep] * 3
        return row
    if fam == "flat":
        return torch.full((V,), 1.5)
    if fam == "quant":
        return (n * 3).round()
    if fam == "zipf":
        rank = torch.randperm(V, generator=gen).float() + 1
        return -1.1 * rank.log()
    if fam == "szero":                                       # quantised, some zeros are -0.0
        row = (n * 3).round()
        zero = row == 0
        neg = zero & (torch.rand(V, generator=gen) < 0.5)
        row[zero] = 0.0
        row[neg] = -0.0
        return row
    raise KeyError(fam)


@dataclasses.dataclass
class Case:
    name: str
    dtype: torch.dtype
    layout: str              # contig | wide: big[:, :V], big 24 columns wider | offset: big[:, 3:3+V]
    logits: torch.Tensor     # [B, V], stored dtype, CPU
    temperature: torch.Tensor
    top_k: torch.Tensor
    top_p: torch.Tensor
    seeds: torch.Tensor
    families: list

    def place(self, device) -> torch.Tensor:
        """The logits on `device` in the case's layout.  The columns outside the view
        hold +60: a kernel that read one would sample it."""
        B, V = self.logits.shape
        if self.layout == "contig":
            return self.logits.to(device)
        big = torch.full((B, V + 24), 60.0, dtype=self.dtype, device=device)
        view = big[:, :V] if self.layout == "wide" else big[:, 3:3 + V]
        view.copy_(self.logits)
        return view


def _resolve_k(k, V):
    return {"V-1": V - 1, "V": V, "V+5": V + 5}.get(k, k)


def make_case(name: str, dtype_name: str, B: int, V: int, layout: str = "contig",
              start: int = 0) -> Case:
    """Rows cycle through the families (12), the parameter kinds (13), the temperatures (9)
    and the seeds (8) with a running counter from `start`, so that across the matrix every
    family meets every kind and every temperature."""
    dt = DTYPES[dtype_name]
    gen = torch.Generator().manual_seed(1000003 * start + 131 * V + B)
    rows, temp, tk, tp, seeds, fams = [], [], [], [], [], []
    for b in range(B):
        n = start + b
        fam = FAMILIES[n % len(FAMILIES)]
        k, p = KINDS[n % len(KINDS)]
        k = _resolve_k(k, V)
        t = TEMPS[(n + n // 36) % len(TEMPS)]
        row = family_row(fam, V, gen).to(dt)
        if fam == "szero":
            # the k-th largest value is +0.0 (positives, then some of the +0.0 zeros),
            # top_p < 1, and never greedy
            pos = int((row.float() > 0).sum())
            pz = int(((row.float() == 0) & ~torch.signbit(row.float())).sum())
            if pz > 0 and pos + 1 < V:
                k = min(pos + (pz + 1) // 2, V - 1)
            p = (0.5, 0.9, 0.99, _P_BELOW_1)[(n // len(FAMILIES)) % 4]
            if t <= 1e-5:
                t = 0.7
        rows.append(row)
        temp.append(t)
        tk.append(k)
        tp.append(p)
        seeds.append(SEEDS[n % len(SEEDS)] ^ (n // len(SEEDS)) if n >= len(SEEDS)
                     else SEEDS[n])
        fams.append(fam)
    return Case(name, dt, layout, torch.stack(rows), torch.tensor(temp, dtype=torch.float32),
                torch.tensor(tk, dtype=torch.int32), torch.tensor(tp, dtype=torch.float32),
                torch.tensor(seeds, dtype=torch.int64), fams)


# (B, V): S = min(16, CUs / B) workgroups per row on a 256-CU device
#   1, 3, 16  S = 16; V = 8 and 100 leave most workgroups an empty or sub-8 slice
#   17        S = 15: slices start off a multiple of 8
#   256       S = 1: the whole row in one workgroup; V = 40000 is two trips of the
#             four-vector loop, the second partial
#   260       the single-workgroup-threshold kernel
SHAPES = ([(B, V) for B in (1, 3, 16) for V in (8, 100, 1000, 4104, 50257, 128256)] +
          [(17, 1000), (17, 50257), (256, 1000), (256, 40000),
           (260, 100), (260, 1000), (260, 4104)])
LAYOUT_SHAPES = [(B, V) for B in (3, 16) for V in (1000, 50257)]


def case_specs() -> list[tuple]:
    """(name, dtype, B, V, layout, start) of every case, cheap to enumerate."""
    specs, start = [], 0
    for B, V in SHAPES:
        for dn in DTYPES:
            specs.append((f"{dn}-B{B}-V{V}", dn, B, V, "contig", start))
            start += B + 5                       # 5: a different alignment of the cycles
    for B, V in LAYOUT_SHAPES:
        for dn in ("bf16", "f16"):
            for layout in ("wide", "offset"):
                specs.append((f"{dn}-B{B}-V{V}-{layout}", dn, B, V, layout, start))
                start += B + 5
    return specs


CASE_NAMES = [s[0] for s in case_specs()]


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    spec = next(s for s in case_specs() if s[0] == name)
    return make_case(*spec)


@functools.lru_cache(maxsize=None)
def case_verdicts(name: str) -> tuple:
    c = case(name)
    return tuple(judge(c.logits, c.temperature, c.top_k, c.top_p, c.seeds))


assert math.isclose(_P_BELOW_1, 1 - 2 ** -24)
