"""W4A16 (--quantization mxfp4) GEMMs vs the fp8 and bf16 paths on a model's projection shapes.

    python tools/w4_gemm_bench.py [--model llama-3-8b] [--layers 32] [--ms 1,4,16,64]
                                  [--big-ms 128,256] [--mid-ms 128,256,512]
                                  [--out profiles/w4_gemm_vs_fp8.jsonl]

Every shape is timed over ``--layers`` distinct weight copies on graph replays (as in a
decode step the weights stream from HBM, not the 256 MB Infinity Cache), all three sides back
to back in one process.  One JSON line per case:
  M <= 64: K9f's best configuration and the mxfp4 widen path, K9q's best configuration
           measured TWICE (the spread of the two is the noise of the comparison), and the
           bf16 side as the start-up tuner picks it (K9 skinny or hipBLASLt);
  --big-ms (M > 64): the mxfp4 widen + hipBLASLt path against plain bf16 hipBLASLt;
  --mid-ms (64 < M <= 512): K9mf per (cfg, S), with the split-K reduction (gate_up: the SiLU
           epilogue or reduction) in the timing, against widen + hipBLASLt (+ silu_mul), bf16
           hipBLASLt, and K9mq's best (cfg, S) on the same shape, over ``--big-layers`` weights.
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
    ap.add_argument("--ms", default="1,4,16,64")
    ap.add_argument("--big-ms", default="")
    ap.add_argument("--big-layers", type=int, default=8)
    ap.add_argument("--mid-ms", default="")
    ap.add_argument("--gemms", default="qkv,o,gate_up,down")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from kubernetes_gpu_cluster_amd import ops
    from kubernetes_gpu_cluster_amd.models import configs
    from kubernetes_gpu_cluster_amd.ops import gemm
    from kubernetes_gpu_cluster_amd.ops.quant import quantize_fp8_rows, quantize_mxfp4
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
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for name in [g for g in a.gemms.split(",") if g]:
        N, K = shapes[name]
        ws = [torch.randn(N, K, dtype=dt, device=dev) * 0.02 for _ in range(a.layers)]
        q8 = [quantize_fp8_rows(w)[0] for w in ws]
        q4 = [quantize_mxfp4(w)[0] for w in ws]
        gemm.w8_reserve(dev, N * K, dt)
        gemm.clear_plan()
        if ms:
            w8a = gemm.tune_w8(q8, ms, dt, reps=5)
            bf = gemm.tune_skinny(ws, ms, reps=5)
            w4 = gemm.tune_w4(q4, ms, dt, reps=5)
            w8b = gemm.tune_w8(q8, ms, dt, reps=5)
        for M in ms:
            chosen, lib_us, sk_us, _ = bf[(M, N, K)]
            bf_us = sk_us if chosen else lib_us
            w4_chosen, wide_us, k9f_us, k9f_cfg = w4[(M, N, K)]
            k9q = sorted([w8a[(M, N, K)][2], w8b[(M, N, K)][2]])
            emit({"gemm": name, "M": M, "N": N, "K": K, "bf16_path": "K9" if chosen else "hipblaslt",
                  "bf16_us": round(bf_us, 2), "k9q_us": [round(t, 2) for t in k9q],
                  "k9q_cfg": w8b[(M, N, K)][3], "k9f_cfg": k9f_cfg, "k9f_us": round(k9f_us, 2),
                  "w4_widen_us": round(wide_us, 2), "w4_chosen": "K9f" if w4_chosen else "widen",
                  "k9q_spread": round(k9q[1] / k9q[0] - 1, 4),
                  "k9f_speedup_vs_k9q": round(k9q[0] / k9f_us, 3),
                  "k9f_speedup_vs_bf16": round(bf_us / k9f_us, 3),
                  "k9f_weight_TBps": round(N * K * 17 / 32 / k9f_us / 1e6, 2),
                  "k9q_weight_TBps": round(N * K / k9q[0] / 1e6, 2)})
        gemm.clear_plan()
        nb = min(a.big_layers, a.layers)
        for M in big:
            x = torch.randn(M, K, dtype=dt, device=dev)

            def lib():
                for w in ws[:nb]:
                    F.linear(x, w)

            def wide():
                for w in q4[:nb]:
                    gemm.w4_widen_linear(x, w, w.w4_scale)
            lib_us = gemm._time_graphed(lib, 5) * 1e3 / nb
            wide_us = gemm._time_graphed(wide, 5) * 1e3 / nb
            emit({"gemm": name, "M": M, "N": N, "K": K, "bf16_path": "hipblaslt",
                  "bf16_us": round(lib_us, 2), "w4_widen_us": round(wide_us, 2),
                  "widen_slowdown_vs_bf16": round(wide_us / lib_us, 3)})
        mid = [int(m) for m in a.mid_ms.split(",") if m]
        if mid:
            silu = name == "gate_up"
            k = torch.ops.kgc
            gemm.pack_w4_decode_weights([] if silu else q4[:nb], q4[:nb] if silu else [])
            gemm.pack_w8_decode_weights([] if silu else q8[:nb], q8[:nb] if silu else [])
            p4 = [gemm.w4_packed_weight(w, silu) for w in q4[:nb]]
            p8 = [gemm.w8_packed_weight(w, silu) for w in q8[:nb]]
            s8 = [gemm._packed_entry(w, silu)[2] if silu else w.w8_scale for w in q8[:nb]]
        for M in mid:
            x = torch.randn(M, K, dtype=dt, device=dev)
            No = N // 2 if silu else N
            red = torch.empty(M, No, dtype=dt, device=dev)

            def lib():
                for w in ws[:nb]:
                    y = F.linear(x, w)
                    if silu:
                        ops.silu_mul(y, red)

            def wide():
                for w in q4[:nb]:
                    y = gemm.w4_widen_linear(x, w, w.w4_scale)
                    if silu:
                        ops.silu_mul(y, red)

            def kern(launch, cfg, S):
                buf = (torch.empty(S, M, N, dtype=torch.float32, device=dev) if S > 1 else
                       torch.empty(M, No, dtype=dt, device=dev))

                def run():
                    for i in range(nb):
                        launch(buf, i, cfg, 0 if S > 1 else (2 if silu else 1))
                        if S > 1 and silu:
                            k.splitk_reduce_silu(red, buf, True)
                        elif S > 1:
                            k.splitk_reduce(red, buf)
                return gemm._time_graphed(run, 5) * 1e3 / nb
            lib_us = gemm._time_graphed(lib, 5) * 1e3 / nb
            wide_us = gemm._time_graphed(wide, 5) * 1e3 / nb
            f_us = {(c, S): kern(lambda b, i, c, e: k.w4_dgemm(b, x, p4[i], None, c, e), c, S)
                    for c, S in gemm._q_dg_candidates(M, N, K, gemm._w4_dg_tiles())}
            q_us = {(c, S): kern(lambda b, i, c, e: k.w8_dgemm(
                        b, x, p8[i], s8[i] if silu and e == 0 else q8[i].w8_scale, None, c, e), c, S)
                    for c, S in gemm._q_dg_candidates(M, N, K, gemm._w8_dg_tiles())}
            fb, qb = min(f_us, key=f_us.get), min(q_us, key=q_us.get)
            emit({"gemm": name, "M": M, "N": N, "K": K, "consumer": "silu" if silu else "plain",
                  "bf16_us": round(lib_us, 2), "w4_widen_us": round(wide_us, 2),
                  "k9mf_us": {f"{c}/{S}": round(t, 2) for (c, S), t in sorted(f_us.items())},
                  "k9mf_best": list(fb), "k9mf_best_us": round(f_us[fb], 2),
                  "k9mq_best": list(qb), "k9mq_best_us": round(q_us[qb], 2),
                  "k9mf_speedup_vs_widen": round(wide_us / f_us[fb], 3),
                  "k9mf_speedup_vs_k9mq": round(q_us[qb] / f_us[fb], 3),
                  "k9mf_speedup_vs_bf16": round(lib_us / f_us[fb], 3)})
        del ws, q8, q4
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
