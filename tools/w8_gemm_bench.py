"""W8A16 (--quantization fp8) GEMMs vs the bf16 paths on a model's projection shapes.

    python tools/w8_gemm_bench.py [--model llama-3-8b] [--layers 32] [--ms 1,8,16,64]
                                  [--big-ms 128,256,4096] [--out profiles/w8_gemm_vs_bf16.jsonl]

Every shape is timed over ``--layers`` distinct weight copies on graph replays (as in a
decode step the weights stream from HBM, not the 256 MB Infinity Cache).  One JSON line
per case:
  M <= 64: K9q's best configuration and the widen path against the bf16 side as the
           start-up tuner picks it (K9 skinny or hipBLASLt);
  M  > 64: the widen + hipBLASLt path against plain bf16 hipBLASLt;
  --mid-ms (64 < M <= 512, e.g. 128,256,512): the best K9mq configuration against the widen
           path and against the bf16 side as the start-up tuner picks it (K9m or hipBLASLt),
           each with the consumer the engine runs behind it (gate_up: SiLU-and-mul, o / down:
           residual add + RMSNorm, qkv: none / the split-K reduction).
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama-3-8b")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--ms", default="1,8,16,64")
    ap.add_argument("--big-ms", default="128,256,4096")
    ap.add_argument("--big-layers", type=int, default=8)
    ap.add_argument("--mid-ms", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from kubernetes_gpu_cluster_amd.models import configs
    from kubernetes_gpu_cluster_amd.ops import gemm
    from kubernetes_gpu_cluster_amd.ops.quant import quantize_fp8_rows
    from kubernetes_gpu_cluster_amd.utils.gemm_tuning import enable_tuned_gemms
    enable_tuned_gemms(a.model, 1)
    c = configs.PRESETS[a.model]
    H, d = c.hidden_size, c.head_dim
    shapes = {"qkv": ((c.num_heads + 2 * c.num_kv_heads) * d, H), "o": (H, c.num_heads * d),
              "gate_up": (2 * c.intermediate_size, H), "down": (H, c.intermediate_size)}
    dev = torch.device("cuda")
    dt = torch.bfloat16
    ms = [int(m) for m in a.ms.split(",") if m]
    big = [int(m) for m in a.big_ms.split(",") if m]
    mid = [int(m) for m in a.mid_ms.split(",") if m]
    kinds = {"qkv": "plain", "o": "tail", "gate_up": "silu", "down": "tail"}
    out = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for name, (N, K) in shapes.items():
        ws = [torch.randn(N, K, dtype=dt, device=dev) * 0.02 for _ in range(a.layers)]
        q = [quantize_fp8_rows(w) for w in ws]
        gemm.w8_reserve(dev, N * K, dt)
        gemm.clear_plan()
        bf = gemm.tune_skinny(ws, ms, reps=5) if ms else {}
        w8 = gemm.tune_w8([w for w, _ in q], ms, dt, reps=5) if ms else {}
        for M in ms:
            chosen, lib_us, sk_us, sk_cfg = bf[(M, N, K)]
            w8_chosen, wide_us, k9q_us, k9q_cfg = w8[(M, N, K)]
            bf_us = sk_us if chosen else lib_us
            emit({"gemm": name, "M": M, "N": N, "K": K, "bf16_path": "K9" if chosen else "hipblaslt",
                  "bf16_cfg": chosen, "bf16_us": round(bf_us, 2), "hipblaslt_us": round(lib_us, 2),
                  "k9q_cfg": k9q_cfg, "k9q_us": round(k9q_us, 2), "widen_us": round(wide_us, 2),
                  "w8_chosen": "K9q" if w8_chosen else "widen",
                  "k9q_speedup_vs_bf16": round(bf_us / k9q_us, 3),
                  "k9q_weight_TBps": round(N * K / k9q_us / 1e6, 2),
                  "bf16_weight_TBps": round(N * K * 2 / bf_us / 1e6, 2)})
        gemm.clear_plan()
        if mid:
            kind = kinds[name]
            silu, tail = ({(N, K)} if kind == "silu" else set()), ({(N, K)} if kind == "tail" else set())
            gemm.pack_decode_weights([] if silu else ws, ws if silu else [])
            gemm.pack_w8_decode_weights([] if silu else [w for w, _ in q],
                                        [w for w, _ in q] if silu else [])
            bf = gemm.tune_skinny(ws, mid, reps=5, silu_shapes=silu, tail_shapes=tail)
            w8 = gemm.tune_w8([w for w, _ in q], mid, dt, reps=5, silu_shapes=silu, tail_shapes=tail)
            for M in mid:
                chosen, lib_us, k9m_us, k9m_cfg = bf[(M, N, K, kind)]
                w8_chosen, wide_us, k9mq_us, k9mq_cfg = w8[(M, N, K, kind)]
                bf_us = k9m_us if chosen else lib_us
                emit({"gemm": name, "kind": kind, "M": M, "N": N, "K": K,
                      "bf16_path": "K9m" if chosen else "hipblaslt", "bf16_cfg_S": chosen,
                      "bf16_us": round(bf_us, 2), "hipblaslt_us": round(lib_us, 2),
                      "k9mq_cfg_S": k9mq_cfg, "k9mq_us": round(k9mq_us, 2),
                      "widen_us": round(wide_us, 2), "w8_chosen": "K9mq" if w8_chosen else "widen",
                      "k9mq_speedup_vs_widen": round(wide_us / k9mq_us, 3),
                      "k9mq_speedup_vs_bf16": round(bf_us / k9mq_us, 3),
                      "k9mq_weight_TBps": round(N * K / k9mq_us / 1e6, 2)})
            gemm.clear_plan()
        nb = min(a.big_layers, a.layers)
        for M in big:
            x = torch.randn(M, K, dtype=dt, device=dev)

            def lib():
                for w in ws[:nb]:
                    F.linear(x, w)

            def wide():
                for w, s in q[:nb]:
                    gemm.w8_widen_linear(x, w, s)
            lib_us = gemm._time_graphed(lib, 5) * 1e3 / nb
            wide_us = gemm._time_graphed(wide, 5) * 1e3 / nb
            emit({"gemm": name, "M": M, "N": N, "K": K, "bf16_path": "hipblaslt",
                  "bf16_us": round(lib_us, 2), "widen_us": round(wide_us, 2),
                  "widen_slowdown_vs_bf16": round(wide_us / lib_us, 3)})
        del ws, q
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
