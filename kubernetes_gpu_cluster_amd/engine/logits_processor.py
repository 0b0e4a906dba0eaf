"""Per-request logits processing before sampling (vLLM / OpenAI semantics):

* ``presence_penalty`` / ``frequency_penalty`` over the tokens generated so far;
* ``repetition_penalty`` over prompt + generated tokens (positive logits divided,
  negative multiplied);
* ``logit_bias`` (token id -> additive bias);
* ``min_p``: drop tokens whose probability is below ``min_p`` x the top probability.

Only the rows of requests that use one of these are touched, so the common path
(none used) costs nothing.  Token statistics live on the device, one row per
running-sequence slot.  They are allocated on first use and updated after each sampling
step, so the host never walks token lists for a decode step.  A sequence (re)entering a
slot, on admission or after recompute preemption, has its row rebuilt from its token lists.

On a GPU all of it runs on the K16 HIP kernels (``ops.logits_process``,
``ops.token_stats_update``, ``ops.token_stats_init``): one packed int32 word per (slot,
token) -- bit 31 "in the prompt", low bits the generated count -- and one pinned parameter
block per step, copied without a host wait.  ``KGC_LOGITS_KERNEL=0`` keeps the torch
formulation below (an int32 count row and a prompt bitmap row per slot) on the GPU; on
the CPU it is the only path.
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import ops


def needs_processing(p) -> bool:
    return bool(p.presence_penalty or p.frequency_penalty or p.repetition_penalty != 1.0
                or p.logit_bias or p.min_p > 0.0)


def needs_counts(p) -> bool:
    return bool(p.presence_penalty or p.frequency_penalty or p.repetition_penalty != 1.0)


class LogitsProcessor:
    def __init__(self, max_seqs: int, vocab: int, device: torch.device):
        self.max_seqs, self.vocab, self.device = max_seqs, vocab, device
        self.counts: Optional[torch.Tensor] = None      # [slots, V] int32: generated tokens
        self.prompt_mask: Optional[torch.Tensor] = None  # [slots, V] bool: prompt tokens
        self.kernel = device.type == "cuda" and ops.logits_kernel_enabled()
        self.stats: Optional[torch.Tensor] = None       # K16: [slots, V] int32 packed words
        self._table = (None, None)                      # (the rows list, its LogitsTable)

    def _ensure(self) -> None:
        if self.kernel:
            if self.stats is None:
                self.stats = torch.zeros(self.max_seqs, self.vocab, dtype=torch.int32,
                                         device=self.device)
        elif self.counts is None:
            self.counts = torch.zeros(self.max_seqs, self.vocab, dtype=torch.int32, device=self.device)
            self.prompt_mask = torch.zeros(self.max_seqs, self.vocab, dtype=torch.bool,
                                           device=self.device)

    def init_slot(self, slot: int, prompt: list[int], output: list[int]) -> None:
        """(Re)build a slot's statistics from the sequence's token lists."""
        self._ensure()
        if self.kernel:
            ops.token_stats_init(self.stats, slot, prompt, [t for t in output if t >= 0])
            return
        self.counts[slot].zero_()
        self.prompt_mask[slot].zero_()
        if prompt:
            self.prompt_mask[slot, torch.tensor(prompt, device=self.device)] = True
        out = [t for t in output if t >= 0]
        if out:
            idx = torch.tensor(out, device=self.device)
            self.counts[slot].index_add_(0, idx, torch.ones_like(idx, dtype=torch.int32))

    def _step_table(self, rows: list[tuple]) -> "ops.LogitsTable":
        """The step's parameter table; ``update`` reuses the one ``apply`` built for the
        same rows list."""
        if self._table[0] is rows:
            return self._table[1]
        ps = [x[2] for x in rows]
        slots = [x[1] if needs_counts(x[2]) else -1 for x in rows]
        if any(s >= 0 for s in slots):
            self._ensure()
        table = ops.logits_table(
            [x[0] for x in rows], slots, [p.presence_penalty for p in ps],
            [p.frequency_penalty for p in ps], [p.repetition_penalty for p in ps],
            [p.min_p for p in ps],
            [max(p.temperature, 1e-5) if p.temperature > 0 else 1.0 for p in ps],
            [[(int(k), float(v)) for k, v in p.logit_bias.items()] if p.logit_bias else []
             for p in ps], self.device)
        self._table = (rows, table)
        return table

    def apply(self, logits: torch.Tensor, rows: list[tuple]) -> None:
        """In place on ``logits`` [S, V]; rows = [(row, slot, SamplingParams)]."""
        V = min(logits.shape[-1], self.vocab)
        if self.kernel:
            ops.logits_process(logits, self.stats, self._step_table(rows), V)
            return
        dev = logits.device
        r = torch.tensor([x[0] for x in rows], device=dev)
        sub = logits.index_select(0, r).float()
        pen = [(i, x) for i, x in enumerate(rows) if needs_counts(x[2])]
        if pen:
            self._ensure()
            j = torch.tensor([i for i, _ in pen], device=dev)
            slots = torch.tensor([x[1] for _, x in pen], device=dev)
            pen = [x for _, x in pen]
            cnt = self.counts.index_select(0, slots)[:, :V].float()
            pm = self.prompt_mask.index_select(0, slots)[:, :V]
            pres = torch.tensor([x[2].presence_penalty for x in pen], device=dev)[:, None]
            freq = torch.tensor([x[2].frequency_penalty for x in pen], device=dev)[:, None]
            rep = torch.tensor([x[2].repetition_penalty for x in pen], device=dev)[:, None]
            s = sub.index_select(0, j)[:, :V]
            seen = (cnt > 0) | pm
            s = torch.where(seen & (s > 0), s / rep, torch.where(seen, s * rep, s))
            s = s - freq * cnt - pres * (cnt > 0).float()
            sub[j, :V] = s
        for i, (_, _, p) in enumerate(rows):
            if p.logit_bias:
                ids = torch.tensor([int(k) for k in p.logit_bias], device=dev)
                vals = torch.tensor([float(v) for v in p.logit_bias.values()], device=dev)
                ok = ids < V
                sub[i].index_add_(0, ids[ok], vals[ok])
        mp = [(i, p.min_p, p.temperature) for i, (_, _, p) in enumerate(rows) if p.min_p > 0]
        if mp:
            j = torch.tensor([m[0] for m in mp], device=dev)
            t = torch.tensor([max(m[2], 1e-5) if m[2] > 0 else 1.0 for m in mp], device=dev)[:, None]
            pm = torch.tensor([m[1] for m in mp], device=dev)[:, None]
            s = sub.index_select(0, j)
            prob = torch.softmax(s / t, dim=-1)
            keep = prob >= pm * prob.max(dim=-1, keepdim=True).values
            sub[j] = torch.where(keep, s, torch.full_like(s, float("-inf")))
        logits.index_copy_(0, r, sub.to(logits.dtype))

    def update(self, rows: list[tuple], sampled: torch.Tensor) -> None:
        """Count each penalised row's new token (device scatter, no host sync)."""
        if self.kernel:
            table = self._step_table(rows)
            if table.any_slot:
                ops.token_stats_update(self.stats, table, sampled)
            return
        pen = [(x[0], x[1]) for x in rows if needs_counts(x[2])]
        if not pen:
            return
        dev = sampled.device
        j = torch.tensor([p[0] for p in pen], device=dev)
        slots = torch.tensor([p[1] for p in pen], device=dev)
        tok = sampled.index_select(0, j).clamp_(0, self.vocab - 1)
        self.counts.index_put_((slots, tok), torch.ones_like(tok, dtype=torch.int32), accumulate=True)
