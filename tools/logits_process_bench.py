"""K16 logits processing against the torch formulation (the ``KGC_LOGITS_KERNEL=0`` code path
of engine/logits_processor.py), through the engine's own ``LogitsProcessor.apply`` + ``update``
on the same logits.

    python tools/logits_process_bench.py [--vocab 128256] [--rows 1,16,256]
                                         [--out profiles/logits_process_kernel_vs_torch.jsonl]

Both run in one process, alternating call by call after a warm-up.  A call is timed with a
host clock around ``apply`` + ``update`` and a device synchronise, so the torch path's
host-side tensor constructions (which the host waits for) count, as they do in a decode step.
Every row carries (a) penalties only, or (b) penalties + 16 bias entries + min_p.  The peak of
``torch.cuda.max_memory_allocated`` above the resident logits and statistics is recorded for
each, and the bytes of the statistics themselves.  One JSON line per (rows, case).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--rows", default="1,16,256")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from kubernetes_gpu_cluster_amd import ops
    from kubernetes_gpu_cluster_amd.engine.logits_processor import LogitsProcessor
    from kubernetes_gpu_cluster_amd.engine.sequence import SamplingParams
    ops.load_extension(strict=True)
    dev, V = torch.device("cuda"), a.vocab
    g = torch.Generator().manual_seed(0)
    cases = {"penalties": dict(presence_penalty=0.5, frequency_penalty=0.5, repetition_penalty=1.1),
             "penalties+bias16+min_p": dict(presence_penalty=0.5, frequency_penalty=0.5,
                                            repetition_penalty=1.1, min_p=0.05, temperature=0.8,
                                            logit_bias={1000 * i + 7: 1.5 for i in range(16)})}
    lines = []
    for S in [int(x) for x in a.rows.split(",")]:
        base = (torch.randn(S, V, generator=g) * 3).to(torch.bfloat16).to(dev)
        sampled = torch.randint(V, (S,), generator=g).to(dev)
        procs = {}
        for kernel in (True, False):
            torch.cuda.synchronize()
            m0 = torch.cuda.memory_allocated()
            p = LogitsProcessor(S, V, dev)
            p.kernel = kernel
            for s in range(S):       # 64 prompt tokens and 192 generated ones per sequence
                p.init_slot(s, torch.randint(V, (64,), generator=g).tolist(),
                            torch.randint(V, (192,), generator=g).tolist())
            torch.cuda.synchronize()
            procs[kernel] = (p, torch.cuda.memory_allocated() - m0)
        for name, kw in cases.items():
            params = SamplingParams(max_tokens=1, **kw)
            logits = base.clone()

            def call(kernel):
                rows = [(i, i, params) for i in range(S)]      # a fresh list, as a plan's is
                t0 = time.perf_counter()
                procs[kernel][0].apply(logits, rows)
                procs[kernel][0].update(rows, sampled)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e6

            def peak(kernel):
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                m = torch.cuda.memory_allocated()
                call(kernel)
                return torch.cuda.max_memory_allocated() - m

            for _ in range(a.warmup):
                logits.copy_(base), call(True)
                logits.copy_(base), call(False)
            tk, tt = [], []
            for _ in range(a.iters):                   # alternating, same process, same logits
                logits.copy_(base)
                torch.cuda.synchronize()
                tk.append(call(True))
                logits.copy_(base)
                torch.cuda.synchronize()
                tt.append(call(False))
            rec = {"op": "logits_process apply+update", "S": S, "V": V, "dtype": "bf16", "case": name,
                   "kernel_us": round(statistics.median(tk), 1),
                   "torch_us": round(statistics.median(tt), 1),
                   "kernel_us_min": round(min(tk), 1), "torch_us_min": round(min(tt), 1),
                   "speedup": round(statistics.median(tt) / statistics.median(tk), 2),
                   "kernel_peak_bytes": peak(True), "torch_peak_bytes": peak(False),
                   "kernel_stats_bytes": procs[True][1], "torch_stats_bytes": procs[False][1],
                   "logits_bytes": logits.numel() * 2, "iters": a.iters,
                   "device": torch.cuda.get_device_name(0)}
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
        del procs
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
