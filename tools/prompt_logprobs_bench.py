"""K15 prompt-logprobs kernel against the torch formulation the runner uses for sampled rows
(``log_softmax(float)`` + ``gather`` + ``topk``), on the same logits.

    python tools/prompt_logprobs_bench.py [--vocab 128256] [--rows 512,64] [--ks 1,20]
                                          [--out profiles/prompt_logprobs_kernel_vs_torch.jsonl]

Both run in one process, alternating call by call after a warm-up, each timed with device
events; the peak of ``torch.cuda.max_memory_allocated`` above the resident logits is recorded
for each.  One JSON line per (rows, k).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_formulation(logits, targets, k):
    lsm = torch.log_softmax(logits.float(), dim=-1)
    tok = lsm.gather(1, targets.view(-1, 1)).view(-1)
    topv, topi = lsm.topk(max(k, 1), dim=-1)
    return tok, topv, topi


def timed(fn, ev0, ev1):
    ev0.record()
    out = fn()
    ev1.record()
    ev1.synchronize()
    return ev0.elapsed_time(ev1) * 1e3, out          # us


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--rows", default="512,64")
    ap.add_argument("--ks", default="1,20")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from kubernetes_gpu_cluster_amd import ops
    ops.load_extension(strict=True)
    dev = torch.device("cuda")
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    lines = []
    for R in [int(x) for x in a.rows.split(",")]:
        logits = (torch.randn(R, a.vocab, device=dev) * 3).to(torch.bfloat16)
        targets = torch.randint(a.vocab, (R,), device=dev)
        for k in [int(x) for x in a.ks.split(",")]:
            kern = lambda: ops.prompt_logprobs(logits, targets, k)          # noqa: E731
            ref = lambda: torch_formulation(logits, targets, k)            # noqa: E731
            for _ in range(a.warmup):
                kern()
                ref()
            tk, tt = [], []
            for _ in range(a.iters):                   # alternating, same process, same logits
                tk.append(timed(kern, ev0, ev1)[0])
                tt.append(timed(ref, ev0, ev1)[0])
            got, want = kern(), ref()
            err = (got[0] - want[0]).abs().max().item()
            rec = {"op": "prompt_logprobs", "R": R, "V": a.vocab, "dtype": "bf16", "k": k,
                   "kernel_us": round(statistics.median(tk), 1),
                   "torch_us": round(statistics.median(tt), 1),
                   "kernel_us_min": round(min(tk), 1), "torch_us_min": round(min(tt), 1),
                   "speedup": round(statistics.median(tt) / statistics.median(tk), 2),
                   "kernel_peak_bytes": peak_bytes(kern), "torch_peak_bytes": peak_bytes(ref),
                   "logits_bytes": logits.numel() * 2, "iters": a.iters,
                   "max_abs_diff_token_logprob": err,
                   "device": torch.cuda.get_device_name(0)}
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
