"""K9a (--quantization fp8_w8a8: act_quant_fp8 + w8a8_gemm) against the path it replaces
(w8_widen + hipBLASLt) and against hipBLASLt on an unquantised bf16 weight, on a model's
projection shapes at prefill row counts.

    python tools/w8a8_gemm_bench.py [--model llama-3-8b] [--ms 128,512,2048,8192,16384]
                                    [--layers 4] [--rounds 5] [--out profiles/w8a8_gemm_vs_widen.jsonl]

The three sides alternate round by round in one process on one GPU, each round a graph
replay over ``--layers`` distinct weight copies after a warm-up; the median round decides.
K9a is timed under every tile configuration (quantiser included each time) and under the
fixed rule the engine uses (``k9a_rule_cfg``).  Every side's output is compared with the
float64 product of the operands it was given before anything is timed (the figure goes into
the line; a side off by more than a few bf16 roundings stops the run).  One JSON line per
(projection, M): times in us per call, and K9a's dense rate counted as 2 M N K operations.
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
    ap.add_argument("--ms", default="128,512,2048,8192,16384")
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from kubernetes_gpu_cluster_amd.models import configs
    from kubernetes_gpu_cluster_amd.ops import gemm
    from kubernetes_gpu_cluster_amd.ops.quant import mark_act_fp8, quantize_fp8_rows
    from kubernetes_gpu_cluster_amd.utils.gemm_tuning import enable_tuned_gemms
    if not torch.cuda.is_available():
        raise SystemExit("w8a8_gemm_bench: no GPU; nothing is measured without one")
    enable_tuned_gemms(a.model, 1)
    c = configs.PRESETS[a.model]
    H, d = c.hidden_size, c.head_dim
    shapes = {"qkv": ((c.num_heads + 2 * c.num_kv_heads) * d, H), "o": (H, c.num_heads * d),
              "gate_up": (2 * c.intermediate_size, H), "down": (H, c.intermediate_size)}
    dev, dt = torch.device("cuda"), torch.bfloat16
    A8 = gemm.W8A8
    tiles = A8.a8_tiles()
    out = open(a.out, "w") if a.out else None
    for name, (N, K) in shapes.items():
        ws = [torch.randn(N, K, dtype=dt, device=dev) * 0.02 for _ in range(a.layers)]
        q = [mark_act_fp8(quantize_fp8_rows(w)[0]) for w in ws]
        gemm.w8_reserve(dev, N * K, dt)
        for M in (int(m) for m in a.ms.split(",") if m):
            x = torch.randn(M, K, dtype=dt, device=dev)
            y = torch.empty(M, N, dtype=dt, device=dev)
            # correctness first, on the first 64 rows and 256 columns of each side
            xq, xs = quantize_fp8_rows(x[:64])
            wd = q[0][:256].double() * q[0].w8_scale[:256, None].double()
            ref = {"k9a": (xq.double() * xs[:, None].double()) @ wd.t(), "widen": x[:64].double() @ wd.t(),
                   "bf16": x[:64].double() @ ws[0][:256].double().t()}
            got = {"k9a": A8.a8_gemm(x, q[0], q[0].w8_scale), "bf16": F.linear(x, ws[0]),
                   "widen": A8.widen_linear(x, q[0], q[0].w8_scale)}
            # bound: a few bf16 roundings at the largest output (the library may sum bf16
            # split-K partials); the tight check of K9a is tests/test_quant_fp8_w8a8_gpu.py
            err = {k: ((v[:64, :256].double() - ref[k]).abs().max() / ref[k].abs().max()).item()
                   for k, v in got.items()}
            assert max(err.values()) <= 2.0 ** -6, err
            sides = {"widen": lambda: [A8.widen_linear(x, w, w.w8_scale) for w in q],
                     "bf16": lambda: [F.linear(x, w) for w in ws]}
            for cfg in range(len(tiles)):
                sides[f"k9a_cfg{cfg}"] = lambda cfg=cfg: [A8.a8_gemm(x, w, w.w8_scale, None, cfg, y)
                                                          for w in q]
            graphs = {k: gemm._graph_of(fn) for k, fn in sides.items()}
            times = {k: [] for k in graphs}
            for _ in range(a.rounds):
                for k, g in graphs.items():
                    times[k].append(gemm._time(g, a.reps) * 1e3 / a.layers)
            med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
            rule = A8.a8_cfg(M, N)
            k9a = med[f"k9a_cfg{rule}"]
            rec = {"gemm": name, "M": M, "N": N, "K": K, "layers": a.layers, "rounds": a.rounds,
                   "tiles": [list(t) for t in tiles], "k9a_rule_cfg": rule,
                   "k9a_us": round(k9a, 2), "widen_us": round(med["widen"], 2),
                   "bf16_hipblaslt_us": round(med["bf16"], 2),
                   "k9a_cfg_us": [round(med[f"k9a_cfg{c}"], 2) for c in range(len(tiles))],
                   "k9a_speedup_vs_widen": round(med["widen"] / k9a, 3),
                   "k9a_speedup_vs_bf16": round(med["bf16"] / k9a, 3),
                   "k9a_dense_PFLOPs": round(2.0 * M * N * K / k9a / 1e9, 3),
                   "max_err_over_max_out": {k: round(v, 5) for k, v in err.items()},
                   "spread": {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()}}
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del graphs, x, y
        del ws, q
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
