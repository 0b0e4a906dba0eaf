"""Engine-level cost of logits processing: p50-style TPOT of an in-process Llama-3-8B engine
(random weights) at batch 256, once with ``frequency_penalty`` on every request and once with
plain requests, plus the allocator's size of the per-slot token statistics.

    python tools/logits_process_engine_ab.py TREE LABEL

TREE is the checkout to import the package from (this one, or an export of another commit
with the built ``_kgc_ops.so`` copied in), so two commits are compared by running the tool
once per tree in fresh processes, alternating, on the same GPU.  One JSON line per run; the
runs of the K16 change are in ``profiles/logits_process_kernel_vs_torch.jsonl``.

Each case runs two waves of 256 requests (128 prompt tokens, 128 generated); the second is
timed: the mean host time per step over 100 consecutive pure-decode steps at B = 256 (the
step loop runs one step ahead of the device, so over 100 steps this is the device's pace).
"""
import json
import os
import sys
import time

tree, label = os.path.abspath(sys.argv[1]), sys.argv[2]
sys.path.insert(0, tree)

import torch                                                              # noqa: E402
import kubernetes_gpu_cluster_amd as pkg                                  # noqa: E402
from kubernetes_gpu_cluster_amd.engine.config import EngineConfig         # noqa: E402
from kubernetes_gpu_cluster_amd.engine.llm_engine import LLMEngine        # noqa: E402
from kubernetes_gpu_cluster_amd.engine.sequence import SamplingParams     # noqa: E402


def main():
    assert os.path.abspath(pkg.__file__).startswith(tree), pkg.__file__
    eng = LLMEngine(EngineConfig(model="llama-3-8b", dtype="bfloat16", max_model_len=4096,
                                 max_num_seqs=256, max_num_batched_tokens=16384,
                                 random_init=True, seed=0, enable_prefix_caching=False))
    proc = eng.executor.runner.processor
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    proc._ensure()                               # the statistics, as the first penalised step would
    torch.cuda.synchronize()
    stats_bytes = torch.cuda.memory_allocated() - m0
    g = torch.Generator().manual_seed(0)
    res = {}
    for name, kw in (("frequency_penalty", dict(frequency_penalty=0.5)), ("plain", {})):
        for _ in range(2):                       # the first wave warms up
            seqs = [eng.add_request(torch.randint(100, 128000, (128,), generator=g).tolist(),
                                    SamplingParams(temperature=1.0, seed=i, max_tokens=128,
                                                   ignore_eos=True, **kw)) for i in range(256)]
            ts = []
            while eng.has_unfinished():
                eng.step()
                ts.append(time.perf_counter())
            torch.cuda.synchronize()
            assert all(len(s.output_token_ids) == 128 for s in seqs)
        res[name + "_tpot_ms"] = round((ts[-11] - ts[-111]) / 100 * 1e3, 3)
        res[name + "_steps"] = len(ts)
    print(json.dumps({"bench": "engine_ab_logits_process", "tree": label, "model": "llama-3-8b",
                      "batch": 256, "input_len": 128, "output_len": 128, **res,
                      "stats_bytes": stats_bytes, "kernel": getattr(proc, "kernel", False),
                      "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
