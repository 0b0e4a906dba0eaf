// K13w: MoE routing for wide expert counts (Qwen3-MoE: 128 experts, top-8), 64 < E <= 256
// (the fused kernel also takes 16 < E <= 64), k <= 16.  moe.hip's K13 keeps one expert per
// lane (E <= 64) and, fused, every expert's dot product in registers (E <= 16).
//
//   moe_route_wide      : router logits [T, E] (bf16 / f16 / fp32) -> fp32 softmax -> top-k
//                         weights / ids.  One wave per token; lane l owns the C = ceil(E/64)
//                         consecutive experts l*C .. l*C+C-1 (one vector load where the row
//                         is aligned), so "lowest lane among the maxima, lowest local index
//                         in it" is the lowest expert id -- moe_route_kernel's tie rule.
//   moe_gate_route_wide : the router GEMM x [T, H] . wg [E, H]^T on MFMA 16x16x32 fused in
//                         front of the same routing code.  A workgroup owns 16 tokens (MFMA
//                         M) and all E experts as NT = ceil(E/16) accumulator tiles per wave;
//                         its NW waves split K in contiguous H/NW slices.  Both operands are
//                         K-contiguous, so a lane's A and B fragments are each ONE 16-byte
//                         global load of its row (row lane % 16, k-chunk lane / 16): no LDS
//                         staging.  Two k-steps of loads are in flight (registers a0/b0,
//                         a1/b1).  The waves' partial tiles meet in LDS as fp32, in MFMA
//                         fragment order (conflict-free, NT * NW KB: 8 waves up to E = 128,
//                         4 waves above, 64 KB at most), are summed in wave order, rounded to
//                         the activation dtype -- as the unfused GEMM stores its logits --
//                         and routed, 16 / NW tokens per wave.  Rows past T and experts past
//                         E load clamped (always in bounds), are never stored, and padded
//                         experts enter the top-k with probability -1.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; no
// scratch in any instantiation):
//   moe_route_wide_kernel<T, C>            C       2    3    4
//                                          VGPRs  20   22   23      no LDS
//   moe_gate_route_wide_kernel<T, NT, NW>  NT      2    4    6    8     12      16
//                                          NW      8    8    8    8      4       4
//                                          VGPRs  50   71   99  127  182+48  238+64 (+ AGPRs)
//                                          LDS    16   32   48   64     48      64 KB
#include "common.h"
#include "launch.h"

namespace kgc {

// Softmax over the wave's E logits (v[c] = logit of expert lane*C + c, -inf past E), then k
// rounds of arg-max with ties to the lowest expert id; lane j < k ends with pair j.
template <int C>
__device__ __forceinline__ void route_wave(const float (&v)[C], int E, int k, int renorm,
                                           int lane, float* __restrict__ w_row,
                                           int* __restrict__ id_row) {
  float m = v[0];
#pragma unroll
  for (int c = 1; c < C; ++c) m = fmaxf(m, v[c]);
  m = wave_max(m);
  float p[C], s = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    p[c] = lane * C + c < E ? __expf(v[c] - m) : 0.f;
    s += p[c];
  }
  s = wave_sum(s);
#pragma unroll
  for (int c = 0; c < C; ++c) p[c] = lane * C + c < E ? p[c] / s : -1.f;
  float wsel = 0.f, wsum = 0.f;
  int isel = 0;
  for (int j = 0; j < k; ++j) {
    float lb = p[0];
    int li = 0;
#pragma unroll
    for (int c = 1; c < C; ++c)
      if (p[c] > lb) {                       // strict: the lowest local index on a tie
        lb = p[c];
        li = c;
      }
    const float best = wave_max(lb);
    const uint64_t hit = __ballot(lb == best);
    const int src = hit ? __ffsll((unsigned long long)hit) - 1 : 0;   // NaN row: no maximum
    const int e = __shfl(lane * C + li, src, 64);
    if (lane == j) {
      wsel = best;
      isel = e < E ? e : E - 1;
    }
    wsum += best;
#pragma unroll
    for (int c = 0; c < C; ++c)
      if (lane == src && c == li) p[c] = -1.f;
  }
  if (lane < k) {
    w_row[lane] = renorm ? wsel / wsum : wsel;
    id_row[lane] = isel;
  }
}

// ---------------------------------------------------------------------------- route
// vec: the base pointer and the row stride are multiples of C * sizeof(T) bytes
template <typename T, int C>
__global__ __launch_bounds__(256) void moe_route_wide_kernel(const T* __restrict__ logits,
                                                             int64_t stride, int ntok, int E,
                                                             int k, int renorm, int vec,
                                                             float* __restrict__ topk_w,
                                                             int* __restrict__ topk_ids) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= ntok) return;
  const T* row = logits + (int64_t)t * stride;
  const int e0 = lane * C;
  constexpr int B = C * (int)sizeof(T);
  float v[C];
#pragma unroll
  for (int c = 0; c < C; ++c) v[c] = -INFINITY;
  bool loaded = false;
  if constexpr (B == 4 || B == 8 || B == 16) {            // C = 3 rows have no such load
    if (vec && e0 + C <= E) {
      typedef uint32_t words __attribute__((ext_vector_type(B / 4)));
      union {
        words u;
        T h[C];
      } r;
      r.u = *reinterpret_cast<const words*>(row + e0);
#pragma unroll
      for (int c = 0; c < C; ++c) v[c] = to_f<T>(r.h[c]);
      loaded = true;
    }
  }
  if (!loaded) {                                          // the row's tail, or unaligned rows
#pragma unroll
    for (int c = 0; c < C; ++c)
      if (e0 + c < E) v[c] = to_f<T>(row[e0 + c]);
  }
  route_wave<C>(v, E, k, renorm, lane, topk_w + (int64_t)t * k, topk_ids + (int64_t)t * k);
}

// ---------------------------------------------------------------------------- gate + route
template <typename T, int NT, int NW>
__global__ __launch_bounds__(NW * 64) void moe_gate_route_wide_kernel(
    const T* __restrict__ x, int64_t ldx, const T* __restrict__ wg, int H, int E, int ntok, int k,
    int renorm, float* __restrict__ topk_w, int* __restrict__ topk_ids) {
  constexpr int C = NT <= 4 ? 1 : NT <= 8 ? 2 : NT <= 12 ? 3 : 4;   // == ceil(E / 64) for this NT
  __shared__ float part[NW][NT * 4][64];                            // [wave][tile, acc reg][lane]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int t0 = blockIdx.x * 16;

  // operand rows, clamped into the matrices: token t0 + r, expert n * 16 + r of tile n
  const T* xa = x + (int64_t)min(t0 + r, ntok - 1) * ldx + q * 8;
  const T* wb[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) wb[n] = wg + (int64_t)min(n * 16 + r, E - 1) * H + q * 8;

  f32x4 acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  Pack8<T> a0, a1, b0[NT], b1[NT];
  auto load = [&](Pack8<T>& a, Pack8<T>(&b)[NT], int kk) {
    a.u = *reinterpret_cast<const u32x4*>(xa + kk);
#pragma unroll
    for (int n = 0; n < NT; ++n) b[n].u = *reinterpret_cast<const u32x4*>(wb[n] + kk);
  };
  auto fma = [&](const Pack8<T>& a, const Pack8<T>(&b)[NT]) {
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = mfma16x16x32(a.v, b[n].v, acc[n]);
  };
  const int steps = H / (32 * NW);                        // host-checked: H % 256 == 0
  int kk = wave * steps * 32;
  load(a0, b0, kk);
  for (int s = 0; s < steps; s += 2, kk += 64) {
    if (s + 1 < steps) load(a1, b1, kk + 32);
    fma(a0, b0);
    if (s + 1 < steps) {
      if (s + 2 < steps) load(a0, b0, kk + 64);
      fma(a1, b1);
    }
  }
  // acc[n][i] = partial logit of token t0 + q*4 + i, expert n*16 + r
#pragma unroll
  for (int n = 0; n < NT; ++n)
#pragma unroll
    for (int i = 0; i < 4; ++i) part[wave][n * 4 + i][lane] = acc[n][i];
  __syncthreads();

#pragma unroll
  for (int j = 0; j < 16 / NW; ++j) {
    const int tl = wave * (16 / NW) + j;
    const int t = t0 + tl;
    if (t >= ntok) break;                                 // wave-uniform; no barrier follows
    float v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int e = lane * C + c;
      v[c] = -INFINITY;
      if (e < E) {
        const int reg = (e >> 4) * 4 + (tl & 3), src = (tl >> 2) * 16 + (e & 15);
        float sum = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) sum += part[w][reg][src];
        v[c] = to_f(from_f<T>(sum));                      // rounded as the GEMM stores it
      }
    }
    route_wave<C>(v, E, k, renorm, lane, topk_w + (int64_t)t * k, topk_ids + (int64_t)t * k);
  }
}

// ---------------------------------------------------------------------------- launchers
void launch_moe_route_wide(int dtype, const void* logits, int64_t stride, int ntok, int E, int k,
                           bool renorm, float* topk_w, int* topk_ids, hipStream_t s) {
  const dim3 grid((ntok + 3) / 4);
  const int C = (E + 63) / 64;
  const int64_t esz = dtype == DT_F32 ? 4 : 2;
  const int vec = reinterpret_cast<uintptr_t>(logits) % (C * esz) == 0 && stride * esz % (C * esz) == 0;
#define RW(TT, CC)                                                                              \
  moe_route_wide_kernel<TT, CC><<<grid, 256, 0, s>>>((const TT*)logits, stride, ntok, E, k,     \
                                                     renorm, vec, topk_w, topk_ids)
#define RW_C(TT) \
  if (C <= 2) RW(TT, 2); else if (C == 3) RW(TT, 3); else RW(TT, 4);
  if (dtype == DT_BF16) { RW_C(bf16) } else if (dtype == DT_F16) { RW_C(f16) } else { RW_C(float) }
#undef RW_C
#undef RW
}

void launch_moe_gate_route_wide(int dtype, const void* x, int64_t ldx, const void* wg, int H,
                                int E, int ntok, int k, bool renorm, float* topk_w,
                                int* topk_ids, hipStream_t s) {
  const dim3 grid((ntok + 15) / 16);
#define GW(TT, NT, NW)                                                                          \
  moe_gate_route_wide_kernel<TT, NT, NW><<<grid, NW * 64, 0, s>>>(                              \
      (const TT*)x, ldx, (const TT*)wg, H, E, ntok, k, renorm, topk_w, topk_ids)
  // the narrowest tile count that holds E (tiles past E recompute expert E - 1, unused)
#define GW_E(TT)                                                                                \
  if (E <= 32) GW(TT, 2, 8); else if (E <= 64) GW(TT, 4, 8); else if (E <= 96) GW(TT, 6, 8);    \
  else if (E <= 128) GW(TT, 8, 8); else if (E <= 192) GW(TT, 12, 4); else GW(TT, 16, 4);
  if (dtype == DT_BF16) { GW_E(bf16) } else { GW_E(f16) }
#undef GW_E
#undef GW
}

}  // namespace kgc
