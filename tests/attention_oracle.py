"""Float64 oracle of paged attention (CPU only; shares no code with the attention kernels).

Everything is computed from the STORED tensors: the cache contents in the cache dtype
(bf16 / f16 / fp8 e4m3), widened exactly to float64 and multiplied by k_scale / v_scale.

  attend       float64 softmax attention of one query row (or one GQA group of rows) over
               an explicit list of key indices.  Decode, prefill (keys 0 .. abs_pos) and the
               paged gather are built on it, and a mutant is just another key list
               (``mutate``): last / first token dropped, last token twice, chunk [32, 64)
               dropped, a causal leak of a + 1, the V of neighbouring tokens swapped, the
               newest token of the fused decode form taken from the stale cache slot.
  fused_write  float64 q/k RMSNorm + NeoX RoPE + KV write of the fused decode form: the only
               roundings are the ones the operation defines (the split-K slice sum to the
               activation dtype, k / v to the cache element).

Input builders, each returning ``(inputs, expected, tolerance)`` and asserting its own
conditions; random Gaussian q / k / v leave one key about 1 / ctx of the output, below any
usable tolerance, so these inputs make every single key visible:

  census     K = 0, q random: every score is equal and each key weighs exactly 1 / n.
             V[t, kh, j] = 1 iff (t + kh) % d == j, so out[j] = v_scale * count_j / n with
             count_j the attended positions of class j.  P = 1, l = n and the fp32 O
             accumulators are exact integers and the kernels' partials are fp32: the only
             rounding is the output's.  Tolerance: atol 0, rtol 2^-8 (bf16) / 2^-10 (f16).
             For f16 that is twice one output rounding (2^-11).  For bf16 (8 significant
             bits) it is the bound of ONE rounding, half an ulp over the binade's lower end,
             and still sound: the fp32 merge and the v_scale / l multiply add ~2^-22, which
             can push an error past 2^-8 |x| only for x within 2^-14 of a power of two,
             where x rounds to that power and the error is 2^-14 |x|.
             Condition: max count <= 64, so one token more or less moves some channel by
             1 / 64 of itself (less 1 / ctx), 4x the bf16 tolerance; this caps ctx at 64 d.
  needles    filler K ~ 0.05 N(0, 1); query head g of a GQA group is 16 e_{c_g} and its
             needle key 16 e_{c_g} sits at a chosen position per (row, head): score 256
             scale against ~0 for the filler (all values exact in bf16 / f16 / e4m3).  The
             c_g are distinct and all below d / 2, so none is the RoPE partner (c + d / 2)
             of another.  V carries a position code: channel i < 13 is +-1 by bit i of t,
             the rest random.  Tolerance: the suite's ``_tol(dt)``, 6e-2 with an fp8 cache.
             Condition: the oracle's weight on the needle >= 0.99 for every probe.
  poison     (census and needle caches) every cache position at or beyond a row's context
             in its last block, and every block no block table references (block 0, which
             unused table entries name, included) holds the key every query head would
             attend to, 16 sum_g e_{c_g}, with V = 100 -- with an fp8 cache the stored value
             nearest 100 / v_scale, saturated at 448 (e4m3 has no exact 100).  All finite.
  staircase  (prefill, bf16 / f16 caches) K[t, c0] = t % 64, K[t, c1] = t // 64, q[c0] = g,
             q[c1] = 64 g with g = 16 (d = 64) / 32 (d = 128): the score rises by 2.0 / 2.83
             per key, the row at absolute position a puts 0.86 / 0.94 of its mass on key a,
             and the running max grows on every tile.  The oracle sums over the last W keys
             and asserts that the excluded mass is < 1e-12.  Tolerance ``_tol(dt)``.

``compare`` is the comparison of every case, on the GPU and for the mutants alike.
"""
from __future__ import annotations

import functools
import math
import types

import numpy as np
import torch

FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0
EPS = 1e-6
K_SCALE, V_SCALE = 0.5, 0.07        # fp8 caches: 16 / 0.5 = 32 is exact in e4m3
CODE_BITS = 13
WINDOW = 32                         # staircase: keys a - 31 .. a carry all but < 1e-12

MUTANTS = ("drop_last", "drop_first", "dup_last", "drop_chunk", "swap_v")
STALE = "stale"                     # fused decode only
LEAK = "leak"                       # prefill only


# ------------------------------------------------------------------ tolerances
def _suite_tol(dt):
    from test_kernels_gpu import _tol           # the suite's own: not a copy
    return _tol(dt)


def census_tol(dt):
    """Relative only, nothing absolute: see the module docstring for the derivation."""
    return dict(atol=0.0, rtol=2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -10)


def value_tol(dt, fp8):
    return dict(atol=6e-2, rtol=6e-2) if fp8 else _suite_tol(dt)


def compare(got, expected, tol):
    """(elements outside atol + rtol |expected|, largest abs error, largest error relative
    to |expected| over the non-zero expectations); a NaN counts as outside."""
    g = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    e = np.asarray(expected, dtype=np.float64)
    assert g.shape == e.shape, (g.shape, e.shape)
    err = np.abs(g - e)
    bad = ~(err <= tol["atol"] + tol["rtol"] * np.abs(e))
    nz = e != 0
    rel = float(np.nanmax(err[nz] / np.abs(e[nz]))) if nz.any() else 0.0
    return int(bad.sum()), float(np.nanmax(err)) if err.size else 0.0, rel


def rounded(expected, dt):
    """The oracle's answer as the kernel would store it."""
    return torch.from_numpy(np.ascontiguousarray(expected)).to(dt).double().numpy()


# ------------------------------------------------------------------ the oracle
def _attend(q, k, v, scale, kkeys, vkeys):
    kkeys = np.asarray(kkeys, dtype=np.int64)
    vkeys = np.asarray(vkeys, dtype=np.int64)
    if kkeys.shape[-1] == 0:
        return np.zeros(q.shape[:-1] + (v.shape[-1],)), np.zeros(q.shape[:-1] + (0,))
    s = (q @ np.swapaxes(k[kkeys], -1, -2)) * scale
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return p @ v[vkeys], p


def attend(q_row, k, v, scale, keys):
    """softmax(scale q . k[keys]) . v[keys] in float64.  q_row [d] (or [G, d], the rows of
    one GQA group; or [R, G, d] with keys [R, n]); k, v [positions, d]; a key may repeat;
    no keys -> zeros."""
    return _attend(np.asarray(q_row, dtype=np.float64), k, v, scale, keys, keys)[0]


def mutate(keys, name, a):
    """(key list, list of the positions whose V each key takes) of a row whose newest key
    is ``a``.  keys [n] or a window [R, n] with a [R, 1]."""
    keys = np.asarray(keys, dtype=np.int64)
    if name is None or name == STALE:
        return keys, keys
    if name == "swap_v":          # every pair (2i, 2i + 1) inside the context trades V
        return keys, np.where((keys ^ 1) <= a, keys ^ 1, keys)
    if name in ("dup_last", LEAK):
        extra = np.broadcast_to(np.asarray(a + (name == LEAK), dtype=np.int64),
                                keys.shape[:-1] + (1,))
        keys = np.concatenate([keys, extra], -1)
    elif keys.ndim == 2:          # a window a - W + 1 .. a of rows far beyond key 63
        assert keys.min() >= 64
        keys = keys[:, :-1] if name == "drop_last" else keys
    else:
        drop = {"drop_last": keys == a, "drop_first": keys == 0,
                "drop_chunk": (keys >= 32) & (keys < 64)}[name]
        keys = keys[~drop]
    return keys, keys


def widen(t):
    return t.float().double().numpy()


def kv_positions(k_cache, v_cache, bt_row, k_scale=1.0, v_scale=1.0):
    """Float64 K, V [positions, nkv, d] of every position the block-table row spans (its
    unused entries too), from K [nb, nkv, bs, d] and V^T [nb, nkv, bs / 8, d, 8]."""
    blocks = bt_row.long()
    nkv, d = k_cache.shape[1], k_cache.shape[3]
    k = widen(k_cache[blocks]).transpose(0, 2, 1, 3).reshape(-1, nkv, d)
    v = widen(v_cache[blocks]).transpose(0, 2, 4, 1, 3).reshape(-1, nkv, d)
    return k * float(np.float32(k_scale)), v * float(np.float32(v_scale))


def paged_kv(k_cache, v_cache, block_tables, k_scale=1.0, v_scale=1.0):
    """The paged gather: kv_positions of every row."""
    return [kv_positions(k_cache, v_cache, bt, k_scale, v_scale) for bt in block_tables]


def decode(q, kv, ctx, scale, mutant=None, weights_of=None):
    """q [B, nq, d] float64, kv = paged_kv(...) -> [B, nq, d].  ``weights_of`` [B, nq] key
    positions: also returns the softmax weight each (row, head) puts on that key (of the
    unmutated key list)."""
    B, nq, d = q.shape
    nkv = kv[0][0].shape[1]
    G = nq // nkv
    out = np.zeros((B, nq, d))
    w = np.ones((B, nq))
    for b in range(B):
        n = int(ctx[b])
        if n == 0:
            continue
        k, v = kv[b]
        kk, vk = mutate(np.arange(n), mutant, n - 1)
        for h in range(nkv):
            hs = slice(h * G, (h + 1) * G)
            o, p = _attend(q[b, hs], k[:, h], v[:, h], scale, kk, vk)
            out[b, hs] = o
            if weights_of is not None and mutant is None:
                w[b, hs] = p[np.arange(G), weights_of[b, hs]]
    return (out, w) if weights_of is not None else out


def prefill(q, k_cache, v_cache, block_tables, query_lens, seq_lens, scale, k_scale=1.0,
            v_scale=1.0, mutant=None, window=None):
    """q [T, nq, d] float64 -> [T, nq, d]: the row at absolute position a attends keys
    0 .. a.  ``window``: rows from position 64 + window on sum over their last ``window``
    keys only (the caller asserts the excluded mass)."""
    T, nq, d = q.shape
    nkv = k_cache.shape[1]
    G = nq // nkv
    out = np.zeros((T, nq, d))
    r0 = 0
    for i, (ql, L) in enumerate(zip(query_lens, seq_lens)):
        k, v = kv_positions(k_cache, v_cache, block_tables[i], k_scale, v_scale)
        pos = np.arange(L - ql, L)
        far = pos >= 64 + window if window else np.zeros(ql, dtype=bool)
        for h in range(nkv):
            hs = slice(h * G, (h + 1) * G)
            for r in np.nonzero(~far)[0]:
                kk, vk = mutate(np.arange(pos[r] + 1), mutant, pos[r])
                out[r0 + r, hs] = _attend(q[r0 + r, hs], k[:, h], v[:, h], scale, kk, vk)[0]
            if far.any():
                a = pos[far][:, None]
                kk, vk = mutate(a - np.arange(window - 1, -1, -1)[None, :], mutant, a)
                out[r0 + np.nonzero(far)[0], hs] = _attend(q[r0 + np.nonzero(far)[0], hs],
                                                           k[:, h], v[:, h], scale, kk, vk)[0]
        r0 += ql
    return out


def store(x, cache_dtype, scale=1.0):
    """float64 / fp32 value -> cache element (fp8: of x / scale, saturated at +-448)."""
    x = torch.as_tensor(x)
    if cache_dtype == FP8:
        return (x.double() / float(np.float32(scale))).clamp(-FP8_MAX, FP8_MAX).float().to(FP8)
    return x.to(cache_dtype)


def fused_write(qkv, positions, cos_sin, k_cache, v_cache, slots, nq, nkv, d, q_norm_w,
                k_norm_w, eps, act, k_scale=1.0, v_scale=1.0, write=True):
    """The prologue of the fused decode form in float64: qkv [B, N] (or fp32 split-K slices
    [S, B, N], summed and rounded to the activation dtype ``act``), optional per-head q / k
    RMSNorm, NeoX RoPE at ``positions``, k / v rounded to ``act`` and stored at ``slots``
    (-1: nothing) in place.  -> q [B, nq, d] float64 (unrounded)."""
    x = qkv.double().sum(0).to(act) if qkv.dim() == 3 else qkv
    x = widen(x)
    B = x.shape[0]
    q = x[:, :nq * d].reshape(B, nq, d)
    k = x[:, nq * d:(nq + nkv) * d].reshape(B, nkv, d)
    v = x[:, (nq + nkv) * d:(nq + 2 * nkv) * d].reshape(B, nkv, d)
    if q_norm_w is not None:
        q = q / np.sqrt((q * q).mean(-1, keepdims=True) + eps) * widen(q_norm_w)
        k = k / np.sqrt((k * k).mean(-1, keepdims=True) + eps) * widen(k_norm_w)
    cs = widen(cos_sin)[np.asarray(positions)]
    cos, sin = cs[:, None, :d // 2], cs[:, None, d // 2:]

    def rot(t):
        t1, t2 = t[..., :d // 2], t[..., d // 2:]
        return np.concatenate([t1 * cos - t2 * sin, t2 * cos + t1 * sin], -1)

    q, k = rot(q), rot(k)
    bs = k_cache.shape[2]
    for b in range(B if write else 0):
        s = int(slots[b])
        if s < 0:
            continue
        blk, off = s // bs, s % bs
        k_cache[blk, :, off, :] = store(torch.from_numpy(k[b]).to(act), k_cache.dtype, k_scale)
        v_cache[blk, :, off // 8, :, off % 8] = store(torch.from_numpy(v[b]).to(act),
                                                      v_cache.dtype, v_scale)
    return q


# ------------------------------------------------------------------ building blocks
def needle_channels(G, d):
    """c_g: distinct, all below d / 2 (no c_g is another's RoPE partner c + d / 2)."""
    c = [1 + 3 * g for g in range(G)]
    assert len(set(c)) == G and max(c) < d // 2
    return c


def poison_key(G, d):
    k = np.zeros(d, dtype=np.float32)
    k[needle_channels(G, d)] = 16.0
    return k


def census_v(t, nkv, d, v_scale=1.0):
    """[len(t), nkv, d]: v_scale (a stored 1) where (t + kh) % d == j."""
    t = np.asarray(t)
    v = np.zeros((len(t), nkv, d), dtype=np.float32)
    cls = (t[:, None] + np.arange(nkv)[None, :]) % d
    np.put_along_axis(v, cls[:, :, None], np.float32(v_scale), 2)
    return v


def census_expected(keys, kh, d, v_scale):
    """out[j] = v_scale count_j / n for the attended positions ``keys`` of kv head kh."""
    keys = np.asarray(keys, dtype=np.int64)
    if keys.size == 0:
        return np.zeros(d)
    cnt = np.bincount((keys + kh) % d, minlength=d)
    return float(np.float32(v_scale)) * cnt / keys.size


def position_code(t, nkv, d, rng):
    """[len(t), nkv, d]: channel i < 13 is +-1 by bit i of t, the rest N(0, 1)."""
    t = np.asarray(t)
    v = rng.standard_normal((len(t), nkv, d)).astype(np.float32)
    bits = (t[:, None] >> np.arange(CODE_BITS)[None, :]) & 1
    v[:, :, :CODE_BITS] = (2.0 * bits - 1.0)[:, None, :]
    return v


def needle_positions(ctx):
    """The positions a context's probes cycle through: the first tokens, the chunk (32) and
    partition (64) edges at both ends, and 32 k - 1 / 32 k spread over the context."""
    c = [0, 1, 15, 16, 31, 32, 63, 64, ctx - 33, ctx - 32, ctx - 2, ctx - 1]
    nch = ctx // 32
    for k in sorted({max(1, nch * f // 7) for f in range(1, 7)}):
        c += [32 * k - 1, 32 * k]
    out = []
    for p in c:
        if 0 <= p < ctx and p not in out:
            out.append(p)
    return out


class Arena:
    """A paged cache in logical layout [block, offset, kv-head, d], every position poison
    until a row's tokens are put; block 0 is never handed out."""

    def __init__(self, ctxs, nkv, bs, d, rng, k_fill, v_fill, extra=5):
        need = [math.ceil(max(c, 1) / bs) for c in ctxs]
        self.bs, self.nkv, self.d = bs, nkv, d
        nb = 1 + sum(need) + extra
        self.k = np.broadcast_to(k_fill, (nb, bs, nkv, d)).astype(np.float32).copy()
        self.v = np.broadcast_to(v_fill, (nb, bs, nkv, d)).astype(np.float32).copy()
        perm = (1 + rng.permutation(nb - 1)).tolist()
        self.bt = np.zeros((len(ctxs), max(need) + 1), dtype=np.int32)
        at = 0
        for b, n in enumerate(need):
            self.bt[b, :n] = perm[at:at + n]
            at += n

    def put(self, b, t, k=None, v=None):
        t = np.asarray(t)
        blk, off = self.bt[b, t // self.bs], t % self.bs
        if k is not None:
            self.k[blk, off] = k
        if v is not None:
            self.v[blk, off] = v

    def slot(self, b, t):
        return int(self.bt[b, t // self.bs]) * self.bs + t % self.bs

    def caches(self, cache_dtype, k_scale, v_scale):
        nb = self.k.shape[0]
        kc = torch.from_numpy(self.k).permute(0, 2, 1, 3).contiguous()
        vc = torch.from_numpy(self.v).view(nb, self.bs // 8, 8, self.nkv, self.d)
        vc = vc.permute(0, 3, 1, 4, 2).contiguous()
        return store(kc, cache_dtype, k_scale), store(vc, cache_dtype, v_scale)


def _scales(fp8):
    return (K_SCALE, V_SCALE) if fp8 else (1.0, 1.0)


def _cache_dtype(dt, fp8):
    return FP8 if fp8 else dt


# ------------------------------------------------------------------ decode cases
CENSUS_CTX = [1, 31, 32, 33, 63, 64, 65, 129, 300, 1000, 2049]
NEEDLE_CTX = [2049] * 4 + [129, 64, 33, 1]
FUSED_CTX = [1, 17, 64, 65, 1000, 2049, 0]          # the 0: a padding row, slot -1
DTYPES = (torch.bfloat16, torch.float16)
DECODE_Z = (1, 3, 40)
FUSED_Z = (1, 3)

DECODE_CENSUS_CASES = [(dt, d, nq, nkv, bs, fp8) for dt in DTYPES
                       for d, nq, nkv in ((128, 32, 8), (64, 12, 12), (128, 8, 1))
                       for bs in (16, 32) for fp8 in (False, True)]
DECODE_NEEDLE_CASES = [(dt, d, nq, nkv, 16, fp8) for dt in DTYPES
                       for d, nq, nkv in ((128, 32, 8), (128, 28, 4), (64, 8, 2))
                       for fp8 in (False, True)]
FUSED_CASES = [(kind, dt, d, nq, nkv, S, qk_norm, fp8) for kind in ("needle", "census")
               for dt in DTYPES for d, nq, nkv in ((128, 32, 8), (64, 8, 2))
               for S in (0, 3) for qk_norm in (False, True) for fp8 in (False, True)]


def case_id(case):
    return "-".join(str(x).replace("torch.", "") for x in case)


def census_ctx(d):
    return CENSUS_CTX + ([4097] if d == 128 else [])


def _assert_census(ctxs, d):
    worst = max(math.ceil(c / d) for c in ctxs)
    assert worst <= 64, f"census: a class holds {worst} > 64 positions"


@functools.lru_cache(maxsize=4)
def decode_census(dt, d, nq, nkv, bs, fp8):
    ctxs = census_ctx(d)
    _assert_census(ctxs, d)
    rng = np.random.default_rng(1000 + d + nq + bs)
    ks, vs = _scales(fp8)
    ar = Arena(ctxs, nkv, bs, d, rng, poison_key(nq // nkv, d), 100.0)
    for b, c in enumerate(ctxs):
        ar.put(b, np.arange(c), 0.0, census_v(np.arange(c), nkv, d, vs))
    kc, vc = ar.caches(_cache_dtype(dt, fp8), ks, vs)
    q = torch.from_numpy(rng.standard_normal((len(ctxs), nq, d)).astype(np.float32)).to(dt)
    inp = types.SimpleNamespace(q=q, kc=kc, vc=vc, bt=torch.from_numpy(ar.bt),
                                ctx=torch.tensor(ctxs, dtype=torch.int32), scale=d ** -0.5,
                                ks=ks, vs=vs, nq=nq, nkv=nkv, d=d)
    return inp, decode_census_expected(inp), census_tol(dt)


def decode_kv(inp):
    return paged_kv(inp.kc, inp.vc, inp.bt, inp.ks, inp.vs)


def decode_expected(inp, mutant=None, kv=None):
    return decode(widen(inp.q), kv or decode_kv(inp), inp.ctx.tolist(), inp.scale, mutant)


def decode_census_expected(inp, mutant=None):
    """Analytic: the classes of the (mutant's) key list, counted."""
    assert mutant != "swap_v"       # a sum over tokens: invisible, see the mutant test
    G = inp.nq // inp.nkv
    return np.stack([np.stack([census_expected(mutate(np.arange(c), mutant, c - 1)[0], h // G,
                                               inp.d, inp.vs) for h in range(inp.nq)])
                     for c in inp.ctx.tolist()])


@functools.lru_cache(maxsize=4)
def decode_needles(dt, d, nq, nkv, bs, fp8):
    ctxs = NEEDLE_CTX
    rng = np.random.default_rng(2000 + d + nq)
    ks, vs = _scales(fp8)
    G = nq // nkv
    ch = needle_channels(G, d)
    ar = Arena(ctxs, nkv, bs, d, rng, poison_key(G, d), 100.0)
    q = np.zeros((len(ctxs), nq, d), dtype=np.float32)
    where = np.zeros((len(ctxs), nq), dtype=np.int64)
    for b, c in enumerate(ctxs):
        k = (0.05 * rng.standard_normal((c, nkv, d))).astype(np.float32)
        cand = needle_positions(c)
        for h in range(nq):
            where[b, h] = cand[(b * nq + h) % len(cand)]
            q[b, h, ch[h % G]] = 16.0
        for p in set(where[b].tolist()):
            k[p] = 0.0
        for h in range(nq):           # heads of a group sharing a position share the key
            k[where[b, h], h // G, ch[h % G]] = 16.0
        ar.put(b, np.arange(c), k, position_code(np.arange(c), nkv, d, rng))
    kc, vc = ar.caches(_cache_dtype(dt, fp8), ks, vs)
    inp = types.SimpleNamespace(q=torch.from_numpy(q).to(dt), kc=kc, vc=vc,
                                bt=torch.from_numpy(ar.bt),
                                ctx=torch.tensor(ctxs, dtype=torch.int32), scale=d ** -0.5,
                                ks=ks, vs=vs, nq=nq, nkv=nkv, d=d, where=where)
    exp, w = decode(widen(inp.q), decode_kv(inp), ctxs, inp.scale, None, where)
    assert w.min() >= 0.99, f"needle weight {w.min()}"
    return inp, exp, value_tol(dt, fp8)


@functools.lru_cache(maxsize=2)
def fused_decode(kind, dt, d, nq, nkv, S, qk_norm, fp8):
    """The fused decode form: the cache holds tokens 0 .. ctx - 2 and, in the slot of the
    newest token, a stale decoy (needle: the key the launch is about to write, under
    another V code; census: the next class's indicator); the newest token arrives in qkv."""
    from kubernetes_gpu_cluster_amd.ops import reference as ref    # the cos / sin table: data
    ctxs, bs = FUSED_CTX, 16
    if kind == "census":
        _assert_census(ctxs, d)
    rng = np.random.default_rng(3000 + d + nq + S + 7 * qk_norm)
    ks, vs = _scales(fp8)
    G = nq // nkv
    ch = needle_channels(G, d)
    B, N = len(ctxs), (nq + 2 * nkv) * d
    cs = ref.rope_cos_sin_cache(d, 4096, 5e5)
    ar = Arena(ctxs, nkv, bs, d, rng, poison_key(G, d), 100.0)
    x = np.zeros((B, N), dtype=np.float32)
    xq = x[:, :nq * d].reshape(B, nq, d)
    xk = x[:, nq * d:(nq + nkv) * d].reshape(B, nkv, d)
    xv = x[:, (nq + nkv) * d:].reshape(B, nkv, d)
    for b, c in enumerate(ctxs):
        old = np.arange(max(c - 1, 0))
        if kind == "census":
            xq[b] = rng.standard_normal((nq, d))
            ar.put(b, old, 0.0, census_v(old, nkv, d, vs))
            if c:
                xv[b] = census_v([c - 1], nkv, d, vs)[0]
                ar.put(b, [c - 1], 0.0, census_v([c], nkv, d, vs))
        else:
            xq[b].reshape(nkv, G, d)[:, np.arange(G), ch] = 16.0
            xk[b][:, ch] = 16.0
            ar.put(b, old, (0.05 * rng.standard_normal((len(old), nkv, d))).astype(np.float32),
                   position_code(old, nkv, d, rng))
            if c:
                xv[b] = position_code([c - 1], nkv, d, rng)[0]
                stale = position_code([c - 1], nkv, d, rng)
                stale[:, :, :CODE_BITS] *= -1.0
                ar.put(b, [c - 1], None, stale)
    x = torch.from_numpy(x).to(dt)
    if S:       # fp32 split-K slices of unequal weight whose sum is x exactly, in fp32 and in
        # any order (x has <= 11 significant bits, 5 x / 8 <= 14): no rounding to differ on
        qkv = torch.stack([x.float() * 0.5, x.float() * 0.125, x.float() * 0.375]
                          + [torch.zeros(B, N)] * (S - 3))
    else:
        qkv = x
    qn = kn = None
    if qk_norm:  # positive and large enough that the normalised needle still towers
        qn = torch.from_numpy(rng.uniform(2.5, 3.5, d).astype(np.float32)).to(dt)
        kn = torch.from_numpy(rng.uniform(2.5, 3.5, d).astype(np.float32)).to(dt)
    pos = torch.tensor([max(c - 1, 0) for c in ctxs], dtype=torch.int64)
    slots = torch.tensor([ar.slot(b, c - 1) if c else -1 for b, c in enumerate(ctxs)],
                         dtype=torch.int64)
    kc, vc = ar.caches(_cache_dtype(dt, fp8), ks, vs)
    if kind == "needle":    # the decoy key: exactly the key this launch writes
        k1, v1 = kc.clone(), vc.clone()
        fused_write(qkv, pos, cs, k1, v1, slots, nq, nkv, d, qn, kn, EPS, dt, ks, vs)
        for b, c in enumerate(ctxs):
            if c:
                blk, off = int(slots[b]) // bs, int(slots[b]) % bs
                kc[blk, :, off] = k1[blk, :, off]
    inp = types.SimpleNamespace(qkv=qkv, pos=pos, cs=cs, kc=kc, vc=vc, slots=slots, qn=qn,
                                kn=kn, bt=torch.from_numpy(ar.bt),
                                ctx=torch.tensor(ctxs, dtype=torch.int32), scale=d ** -0.5,
                                ks=ks, vs=vs, nq=nq, nkv=nkv, d=d, dt=dt)
    inp.state = fused_state(inp)
    exp, w, inp.kc_after, inp.vc_after = fused_expected(inp, None, True, inp.state)
    if kind == "needle":
        assert w[:-1].min() >= 0.99, f"needle weight {w.min()}"
    return inp, exp, (census_tol(dt) if kind == "census" else value_tol(dt, fp8))


def fused_state(inp, write=True):
    """(float64 q, paged K / V, cache tensors) after the prologue; write=False: the newest
    token is NOT stored, the launch would read the stale slot."""
    kc, vc = inp.kc.clone(), inp.vc.clone()
    q = fused_write(inp.qkv, inp.pos, inp.cs, kc, vc, inp.slots, inp.nq, inp.nkv, inp.d, inp.qn,
                    inp.kn, EPS, inp.dt, inp.ks, inp.vs, write=write)
    return q, paged_kv(kc, vc, inp.bt, inp.ks, inp.vs), kc, vc


def fused_expected(inp, mutant=None, full=False, state=None):
    """Float64 oracle of the whole fused op."""
    q, kv, kc, vc = state or fused_state(inp, mutant != STALE)
    ctx = inp.ctx.tolist()
    newest = np.repeat(np.maximum(np.asarray(ctx) - 1, 0)[:, None], inp.nq, 1)
    out, w = decode(q, kv, ctx, inp.scale, mutant, newest)
    return (out, w, kc, vc) if full else out


# ------------------------------------------------------------------ prefill cases
PREFILL_SEQ = [5, 130, 300, 64, 700, 1030, 17, 2125]
PREFILL_QUERY = [5, 130, 100, 1, 257, 1030, 3, 333]
STAIR_SEQ = [1030, 700, 130]
STAIR_QUERY = [1030, 257, 130]
PREFILL_BS = 16

PREFILL_CENSUS_CASES = [(dt, nq, nkv, d, fp8) for dt in DTYPES
                        for nq, nkv, d in ((32, 8, 128), (16, 4, 64), (8, 1, 128))
                        for fp8 in (False, True)]
STAIRCASE_CASES = [(dt, nq, nkv, d) for dt in DTYPES for nq, nkv, d in ((32, 8, 128), (16, 4, 64))]


def _prefill_inputs(ar, q, seq, query, dt, fp8, **kw):
    ks, vs = _scales(fp8)
    kc, vc = ar.caches(_cache_dtype(dt, fp8), ks, vs)
    qsl = np.concatenate([[0], np.cumsum(query)])
    return types.SimpleNamespace(q=torch.from_numpy(q).to(dt), kc=kc, vc=vc,
                                 bt=torch.from_numpy(ar.bt),
                                 qsl=torch.tensor(qsl, dtype=torch.int32),
                                 sl=torch.tensor(seq, dtype=torch.int32), seq=seq, query=query,
                                 scale=ar.d ** -0.5, ks=ks, vs=vs, nq=q.shape[1], nkv=ar.nkv,
                                 d=ar.d, **kw)


@functools.lru_cache(maxsize=2)
def prefill_census(dt, nq, nkv, d, fp8):
    seq, query = PREFILL_SEQ, PREFILL_QUERY
    _assert_census(seq, d)
    rng = np.random.default_rng(4000 + d + nq)
    vs = _scales(fp8)[1]
    ar = Arena(seq, nkv, PREFILL_BS, d, rng, poison_key(nq // nkv, d), 100.0)
    for i, L in enumerate(seq):
        ar.put(i, np.arange(L), 0.0, census_v(np.arange(L), nkv, d, vs))
    T = sum(query)
    # the RoPE form reads q out of a QKV projection row: q is its first nq d columns
    qkv = rng.standard_normal((T, (nq + 2 * nkv) * d)).astype(np.float32)
    inp = _prefill_inputs(ar, qkv[:, :nq * d].reshape(T, nq, d), seq, query, dt, fp8,
                          qkv=torch.from_numpy(qkv).to(dt))
    return inp, prefill_census_expected(inp), census_tol(dt)


def prefill_census_expected(inp, mutant=None):
    """Analytic: the row at position a counts the classes of keys 0 .. a (of the mutant's
    key list); a leaked key a + 1 enters with its stored V and its weight exp(score) (1 for
    a context token, whose K is 0; the poison beyond the context scores otherwise)."""
    assert mutant != "swap_v"       # a sum over tokens: invisible, see the mutant test
    d, nkv, G = inp.d, inp.nkv, inp.nq // inp.nkv
    vs = float(np.float32(inp.vs))
    out = np.zeros((sum(inp.query), inp.nq, d))
    qf = widen(inp.q)
    r0 = 0
    for i, (ql, L) in enumerate(zip(inp.query, inp.seq)):
        a = np.arange(L - ql, L)
        k = v = None
        if mutant == LEAK:
            k, v = kv_positions(inp.kc, inp.vc, inp.bt[i], inp.ks, inp.vs)
        for kh in range(nkv):
            one = np.eye(d)[(np.arange(L + 1) + kh) % d]                    # class of key t
            cum = np.concatenate([np.zeros((1, d)), np.cumsum(one, 0)])     # keys < t
            cnt, n = cum[a + 1], (a + 1).astype(np.float64)
            if mutant == "drop_last":
                cnt, n = cnt - one[a], n - 1
            elif mutant == "drop_first":
                cnt, n = cnt - one[0], n - 1
            elif mutant == "dup_last":
                cnt, n = cnt + one[a], n + 1
            elif mutant == "drop_chunk":
                lo, hi = np.minimum(a + 1, 32), np.minimum(a + 1, 64)
                cnt, n = cnt - (cum[hi] - cum[lo]), n - (hi - lo)
            for g in range(G):
                h = kh * G + g
                num, den = cnt * vs, n
                if mutant == LEAK:
                    w = np.exp(np.einsum("rd,rd->r", qf[r0:r0 + ql, h], k[a + 1, kh]) * inp.scale)
                    num, den = num + w[:, None] * v[a + 1, kh], den + w
                with np.errstate(invalid="ignore", divide="ignore"):
                    out[r0:r0 + ql, h] = np.where(den[:, None] > 0, num / den[:, None], 0.0)
        r0 += ql
    return out


@functools.lru_cache(maxsize=2)
def prefill_staircase(dt, nq, nkv, d):
    seq, query = STAIR_SEQ, STAIR_QUERY
    rng = np.random.default_rng(5000 + d + nq)
    g = 32.0 if d == 128 else 16.0
    c0, c1 = 5, d // 2 + 9

    def stair(t):
        k = np.zeros((len(t), nkv, d), dtype=np.float32)
        k[:, :, c0], k[:, :, c1] = (t % 64)[:, None], (t // 64)[:, None]
        return k

    # beyond a context the staircase goes on (a leaked key a + 1 outscores key a), V = 100;
    # unreferenced blocks hold its far end
    ar = Arena(seq, nkv, PREFILL_BS, d, rng, stair(np.array([4095]))[0], 100.0)
    for i, L in enumerate(seq):
        cap = math.ceil(L / PREFILL_BS) * PREFILL_BS
        ar.put(i, np.arange(cap), stair(np.arange(cap)))
        ar.put(i, np.arange(L), None, rng.standard_normal((L, nkv, d)).astype(np.float32))
    q = np.zeros((sum(query), nq, d), dtype=np.float32)
    q[:, :, c0], q[:, :, c1] = g, 64 * g
    inp = _prefill_inputs(ar, q, seq, query, dt, False)
    assert torch.equal(inp.q.float(), torch.from_numpy(q))                   # exact in dt
    step = g * inp.scale                                                    # score per key
    assert max(seq) * math.exp(-step * WINDOW) < 1e-12, "staircase: excluded mass"
    return inp, prefill_expected(inp, window=WINDOW), _suite_tol(dt)


def prefill_expected(inp, mutant=None, window=None):
    return prefill(widen(inp.q), inp.kc, inp.vc, inp.bt, inp.query, inp.seq, inp.scale, inp.ks,
                   inp.vs, mutant, window)
