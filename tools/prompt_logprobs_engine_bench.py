"""The price of ``prompt_logprobs`` on prefill: one engine, the bench workload's prompts
(256 x 512 tokens, one generated token each), waves with and without the flag back to back on
the same GPU, alternating.

    python tools/prompt_logprobs_engine_bench.py [--model llama-3-8b] [--num-prompts 256]
        [--input-len 512] [--k 1] [--waves 3] [--out profiles/engine_ab_prompt_logprobs.jsonl]

Dummy weights, eager prefill steps of up to 16384 tokens, prefix caching off (every wave
computes every position).  A wave's time runs from the first add_request to the last first
token.  One JSON line: the per-wave seconds of both arms, their medians, the ratio, and the
prompt positions scored.
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
    ap.add_argument("--model", default="llama-3-8b")
    ap.add_argument("--num-prompts", type=int, default=256)
    ap.add_argument("--input-len", type=int, default=512)
    ap.add_argument("--k", type=int, default=1)
    ap.add_argument("--waves", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from kubernetes_gpu_cluster_amd.engine.config import EngineConfig
    from kubernetes_gpu_cluster_amd.engine.llm_engine import LLMEngine
    from kubernetes_gpu_cluster_amd.engine.sequence import SamplingParams
    eng = LLMEngine(EngineConfig(model=a.model, random_init=True, max_model_len=4096,
                                 max_num_seqs=256, max_num_batched_tokens=16384,
                                 enforce_eager=True, enable_prefix_caching=False))
    g = torch.Generator().manual_seed(0)
    V = eng.mcfg.vocab_size
    prompts = [torch.randint(100, V - 100, (a.input_len,), generator=g).tolist()
               for _ in range(a.num_prompts)]

    def wave(k):
        sp = SamplingParams(temperature=1.0, max_tokens=1, ignore_eos=True, prompt_logprobs=k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, p in enumerate(prompts):
            eng.add_request(p, sp, request_id=f"w{wave.n}-{i}")
        wave.n += 1
        got = 0
        while eng.has_unfinished():
            for o in eng.step():
                got += o.prompt_logprobs is not None and len(o.prompt_logprobs) - 1
        torch.cuda.synchronize()
        return time.perf_counter() - t0, got
    wave.n = 0
    wave(None)
    wave(a.k)                                           # warm-up of both arms
    rows0 = eng.executor.runner.stats["plp_rows"]
    off, on, scored = [], [], 0
    for _ in range(a.waves):
        off.append(wave(None)[0])
        t, n = wave(a.k)
        on.append(t)
        scored = n
    rec = {"bench": "prefill_prompt_logprobs_ab", "model": a.model, "num_prompts": a.num_prompts,
           "input_len": a.input_len, "k": a.k, "waves": a.waves,
           "off_s": [round(x, 4) for x in off], "on_s": [round(x, 4) for x in on],
           "off_median_s": round(statistics.median(off), 4),
           "on_median_s": round(statistics.median(on), 4),
           "ratio": round(statistics.median(on) / statistics.median(off), 3),
           "positions_scored_per_wave": scored,
           "plp_rows": eng.executor.runner.stats["plp_rows"] - rows0,
           "plp_rows_per_call": eng.executor.runner.plp_rows,
           "kv_blocks": eng.num_blocks, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    eng.shutdown()


if __name__ == "__main__":
    main()
