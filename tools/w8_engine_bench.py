"""Decode TPOT and KV blocks of one engine with and without ``--quantization fp8 | mxfp4``.

    python tools/w8_engine_bench.py [--model llama-3-8b] [--batches 1,16] [--quantization fp8|mxfp4]
                                    [--input-len 128] [--output-len 128]

Dummy weights, one GPU, graph-replayed decode.  One JSON line per batch size: the KV blocks
the profile step reports and the mean time per output token of the decode steps (time from
the first to the last generated token / tokens after the first).  Run it once without and
once with ``--quantization fp8``, back to back on the same GPU.  Batches above 64 (128, 256,
512) run the mid-batch decode GEMMs: K9m for bf16 weights, K9mq or the widen path for fp8
ones, and each line then carries the W8 plan of its bucket (``w8_plan``: shape and kind ->
[cfg, S], or "widen").  With ``--quantization mxfp4`` a line of a batch <= 64 carries the W4
plan of its bucket (``w4_plan``: shape -> K9f [mt, nt, nw], or "widen"); a larger batch the
K9mf plan of its bucket (``w4_dg_plan``: shape and kind -> [cfg, S], or "widen").  ``--tag``
labels the lines, ``--out`` appends them to a file.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama-3-8b")
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--quantization", default=None)
    ap.add_argument("--input-len", type=int, default=128)
    ap.add_argument("--output-len", type=int, default=128)
    ap.add_argument("--tag", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocks-only", action="store_true",
                    help="report the KV block count and stop (no graphs, no decode)")
    a = ap.parse_args()
    from kubernetes_gpu_cluster_amd.engine.config import EngineConfig
    from kubernetes_gpu_cluster_amd.engine.llm_engine import LLMEngine
    from kubernetes_gpu_cluster_amd.engine.sequence import SamplingParams
    batches = [int(b) for b in a.batches.split(",")]
    eng = LLMEngine(EngineConfig(model=a.model, random_init=True, quantization=a.quantization,
                                 max_model_len=4096, max_num_seqs=max(256, max(batches)),
                                 max_num_batched_tokens=16384, cuda_graph_max_bs=max(batches),
                                 enforce_eager=a.blocks_only))
    base = {"model": a.model, "quantization": a.quantization, "kv_blocks": eng.num_blocks,
            "weights_gb": round(sum(p.numel() * p.element_size()
                                    for p in eng.executor.runner.model.parameters()) / 1e9, 2)}
    if a.tag:
        base["tag"] = a.tag

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    if a.blocks_only:
        emit(base)
        return
    from kubernetes_gpu_cluster_amd.ops import gemm
    w8_plan = getattr(gemm, "w8_dg_plan", dict)()
    g = torch.Generator().manual_seed(0)
    for B in batches:
        for rep in range(2):        # the first pass warms up
            seqs = [eng.add_request(torch.randint(100, 100000, (a.input_len,), generator=g).tolist(),
                                    SamplingParams(temperature=0.0, max_tokens=a.output_len,
                                                   ignore_eos=True)) for _ in range(B)]
            t_first = None
            while eng.has_unfinished():
                eng.step()
                if t_first is None and all(len(s.output_token_ids) >= 1 for s in seqs):
                    torch.cuda.synchronize()
                    t_first, n_first = time.perf_counter(), min(len(s.output_token_ids) for s in seqs)
            torch.cuda.synchronize()
            t_end = time.perf_counter()
        tpot = (t_end - t_first) / (a.output_len - n_first) * 1e3
        rec = dict(base, batch=B, tpot_ms=round(tpot, 3))
        if a.quantization == "fp8" and B > 64:
            rec["w8_plan"] = {f"{N}x{K}:{kind}": list(v) if v else "widen"
                              for (M, N, K, kind), v in sorted(w8_plan.items()) if M == B}
        if a.quantization == "mxfp4" and B > 64:
            rec["w4_dg_plan"] = {f"{N}x{K}:{kind}": list(v) if v else "widen"
                                 for (M, N, K, kind), v in
                                 sorted(getattr(gemm, "w4_dg_plan", dict)().items()) if M == B}
        if a.quantization == "mxfp4" and B <= 64:
            rec["w4_plan"] = {f"{N}x{K}": list(v) if v else "widen"
                              for (M, N, K), v in sorted(gemm.w4_plan().items()) if M == B}
            rec["w4_silu_plan"] = {f"{N}x{K}": list(v) if v else "widen"
                                   for (M, N, K), v in sorted(gemm.w4_silu_plan().items()) if M == B}
        emit(rec)


if __name__ == "__main__":
    main()
