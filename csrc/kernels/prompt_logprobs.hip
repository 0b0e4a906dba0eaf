// K15 prompt logprobs: log-softmax value of one target column per row, plus the k best
// columns of the row, from the LM-head logits [R, Vloc] of R prompt positions -- without
// ever writing an [R, V] intermediate.
//
// Stage 1 (plp_partial_kernel, grid (R, S), 256 threads): the S workgroups of a row split
//   its valid columns [0, ncols).  A workgroup reads its slice from HBM once (16-byte
//   vector loads for every dtype; the unaligned head and tail of the slice as scalars, so
//   rows at any element offset and stride take the vector path), stages it in LDS as fp32
//   (at most PLP_CAP columns) and writes one record of 3 + 2k words:
//     m = max, s = sum exp(x - m), t = the target's logit (-inf: not in this slice),
//     k candidates (value, global column id), best first.
//   Candidates: k rounds of block arg-max.  Each thread keeps the best of the columns it
//   owns and each wave the best of its threads; after a round only the winner's owner needs
//   a new best -- its best column AFTER the winner in the order below, found by its wave,
//   one column per lane -- so LDS stays read-only, -inf columns are ordinary candidates, and
//   a round costs one barrier.
// Stage 2 (plp_merge_kernel, one wave per row): any number of records of a row ->
//   lse = M + log sum s_i exp(m_i - M), token logprob t - lse, the k best candidates
//   overall as value - lse; or (as_record) one merged record, which a TP rank all-gathers
//   instead of its logits.  Empty records (m = -inf, s = 0) contribute nothing; a row
//   of empty records gives -inf, not NaN.
//
// Order (the same in ops/reference.py and the tests' float64 oracle): value descending as
// floats (-0.0 == +0.0), equal values by ascending global column id; fewer than k valid
// columns: the tail is (id -1, -inf).  Column ids are unique over a row's records, so
// "the best candidate after the previous one" needs no removal marks.
//
// hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage (the KGC_DEBUG
// build compiles the same code):
//   plp_partial_kernel<bf16 / f16>  33 VGPR  43 SGPR  LDS 32864 B  scratch 0  4 waves/SIMD
//   plp_partial_kernel<float>       56 VGPR  43 SGPR  LDS 32864 B  scratch 0  4 waves/SIMD
//   plp_merge_kernel                28 VGPR  58 SGPR  LDS     0 B  scratch 0  8 waves/SIMD
// (4 workgroups of 4 waves per CU, bounded by the LDS stage)
#include "common.h"
#include "launch.h"
#include <algorithm>

namespace kgc {

constexpr int PLP_NT = 256;
constexpr int PLP_CAP = 8192;          // columns a workgroup stages (32 KB of LDS as fp32)
constexpr int PLP_NONE = 0x7fffffff;   // "no candidate"
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

// is candidate (v2, i2) ahead of (v, i) in the order?
__device__ __forceinline__ bool plp_ahead(float v2, int i2, float v, int i) {
  return i2 != PLP_NONE && (i == PLP_NONE || v2 > v || (v2 == v && i2 < i));
}
// is (v, i) strictly behind (pv, pi)?  (pi == -1: nothing selected yet)
__device__ __forceinline__ bool plp_behind(float v, int i, float pv, int pi) {
  return pi < 0 || v < pv || (v == pv && i > pi);
}
__device__ __forceinline__ void plp_wave_best(float& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(v, o, 64);
    const int i2 = __shfl_xor(i, o, 64);
    if (plp_ahead(v2, i2, v, i)) { v = v2; i = i2; }
  }
}

template <typename T>
__global__ __launch_bounds__(PLP_NT) void plp_partial_kernel(
    float* __restrict__ rec, const T* __restrict__ logits, int64_t row_stride,
    const int64_t* __restrict__ targets, int vocab_off, int ncols, int k) {
  constexpr int EPV = 16 / (int)sizeof(T);           // elements per 16-byte vector
  __shared__ __attribute__((aligned(16))) float x[PLP_CAP + 4];
  __shared__ float red_v[PLP_NT / 64];
  __shared__ int red_i[PLP_NT / 64];
  const int r = blockIdx.x, y = blockIdx.y, S = gridDim.y, tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  const int lo = (int)((int64_t)ncols * y / S);
  const int len = min((int)((int64_t)ncols * (y + 1) / S) - lo, PLP_CAP);   // host: <= PLP_CAP
  const T* src = logits + (int64_t)r * row_stride + lo;
  const int W = 3 + 2 * k;
  float* out = rec + ((int64_t)r * S + y) * W;

  // ---- HBM -> LDS, once.  head: scalars up to the first 16-byte boundary; the staged
  // copy starts at x[pad] so that every vector lands 16-byte aligned in LDS too
  const int mis = (int)(reinterpret_cast<uintptr_t>(src) & 15) / (int)sizeof(T);
  const int head = min(len, (EPV - mis) % EPV);
  const int nvec = (len - head) / EPV;
  const int pad = (4 - (head & 3)) & 3;
  float* xs = x + pad;
  if (tid < head) xs[tid] = to_f(src[tid]);
  for (int v = tid; v < nvec; v += PLP_NT) {
    const u32x4 raw = *reinterpret_cast<const u32x4*>(src + head + v * EPV);
    float* d = xs + head + v * EPV;
    if constexpr (sizeof(T) == 2) {
      Pack8<T> p;
      p.u = raw;
      *reinterpret_cast<f32x4*>(d) = f32x4{to_f(p.h[0]), to_f(p.h[1]), to_f(p.h[2]), to_f(p.h[3])};
      *reinterpret_cast<f32x4*>(d + 4) = f32x4{to_f(p.h[4]), to_f(p.h[5]), to_f(p.h[6]), to_f(p.h[7])};
    } else {
      *reinterpret_cast<u32x4*>(d) = raw;
    }
  }
  for (int i = head + nvec * EPV + tid; i < len; i += PLP_NT) xs[i] = to_f(src[i]);
  __syncthreads();

  // ---- max, then sum exp(x - max), over the columns this thread owns (tid, tid + NT, ..)
  float bv = 0.f;
  int bi = PLP_NONE;
  for (int j = tid; j < len; j += PLP_NT) {
    const float v = xs[j];
    if (plp_ahead(v, j, bv, bi)) { bv = v; bi = j; }
  }
  float m = bi == PLP_NONE ? -INFINITY : bv;
  m = block_max<PLP_NT>(m, red_v);
  float s = 0.f;
  if (m > -INFINITY) {
    for (int j = tid; j < len; j += PLP_NT) s += __builtin_amdgcn_exp2f((xs[j] - m) * LOG2E);
  }
  s = block_sum<PLP_NT>(s, red_v);
  if (tid == 0) {
    const int64_t tl = targets[r] - (int64_t)vocab_off - (int64_t)lo;
    out[0] = m;
    out[1] = s;
    out[2] = (tl >= 0 && tl < (int64_t)len) ? xs[(int)tl] : -INFINITY;
  }

  // ---- k rounds of block arg-max; (bv, bi) is this thread's best column not yet taken,
  // (mv, mi) its wave's.  A round reads the PLP_NT / 64 wave bests, and only the winner's
  // wave has work: its lanes rescan the owner thread's columns (one each: PLP_CAP / PLP_NT
  // <= 64) for the best one behind the winner, and reduce again.  The wave bests ping-pong
  // between two LDS rows, so a round costs one barrier.
  static_assert(PLP_CAP / PLP_NT <= 64 && (PLP_NT & (PLP_NT - 1)) == 0, "rescan: one column per lane");
  __shared__ float top_v[2][PLP_NT / 64];
  __shared__ int top_i[2][PLP_NT / 64];
  float mv = bv;
  int mi = bi;
  plp_wave_best(mv, mi);
  if (lane == 0) { top_v[0][w] = mv; top_i[0][w] = mi; }
  __syncthreads();
  for (int q = 0; q < k; ++q) {
    const int cur = q & 1;
    float wv = top_v[cur][0];
    int wi = top_i[cur][0];
#pragma unroll
    for (int j = 1; j < PLP_NT / 64; ++j)
      if (plp_ahead(top_v[cur][j], top_i[cur][j], wv, wi)) { wv = top_v[cur][j]; wi = top_i[cur][j]; }
    if (tid == 0) {
      out[3 + q] = wi == PLP_NONE ? -INFINITY : wv;
      out[3 + k + q] = __int_as_float(wi == PLP_NONE ? -1 : vocab_off + lo + wi);
    }
    if (wi != PLP_NONE) {                       // (block-uniform: every thread read the same)
      const int ot = wi & (PLP_NT - 1);         // the owner thread of column wi
      if (w == (ot >> 6)) {
        const int j = ot + PLP_NT * lane;
        float cv = 0.f;
        int ci = PLP_NONE;
        if (j < len) {
          const float c = xs[j];
          if (plp_behind(c, j, wv, wi)) { cv = c; ci = j; }
        }
        plp_wave_best(cv, ci);
        if (tid == ot) { bv = cv; bi = ci; }
        mv = bv;
        mi = bi;
        plp_wave_best(mv, mi);
      }
    }
    if (lane == 0) { top_v[cur ^ 1][w] = mv; top_i[cur ^ 1][w] = mi; }
    __syncthreads();
  }
}

// One wave per row: reduce the row's N records (W = 3 + 2k words each, rec[r][n][..]).
// as_record: out_rec[r] = the merged record; otherwise tok_lp / top_lp / top_id.
__global__ __launch_bounds__(64) void plp_merge_kernel(
    float* __restrict__ tok_lp, float* __restrict__ top_lp, int* __restrict__ top_id,
    float* __restrict__ out_rec, const float* __restrict__ rec, int N, int k) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const int W = 3 + 2 * k;
  const float* base = rec + (int64_t)r * N * W;
  float M = -INFINITY, t = -INFINITY;
  for (int n = lane; n < N; n += 64) {
    M = fmaxf(M, base[(int64_t)n * W]);
    t = fmaxf(t, base[(int64_t)n * W + 2]);
  }
  M = wave_max(M);
  t = wave_max(t);
  float s = 0.f;
  for (int n = lane; n < N; n += 64) {
    const float mi = base[(int64_t)n * W];
    if (mi > -INFINITY) s += base[(int64_t)n * W + 1] * __builtin_amdgcn_exp2f((mi - M) * LOG2E);
  }
  s = wave_sum(s);
  const float lse = M + __builtin_amdgcn_logf(s) * LN2;
  // -inf stays -inf whatever lse is (an all-empty row has lse = -inf: no inf - inf)
  auto lp = [&](float v) { return (v == -INFINITY || !(s > 0.f)) ? -INFINITY : v - lse; };
  if (lane == 0) {
    if (out_rec != nullptr) {
      float* o = out_rec + (int64_t)r * W;
      o[0] = M;
      o[1] = s;
      o[2] = t;
    } else {
      tok_lp[r] = lp(t);
    }
  }
  float pv = 0.f;
  int pi = -1;
  bool exhausted = false;
  for (int q = 0; q < k; ++q) {
    float bv = 0.f;
    int bi = PLP_NONE;
    if (!exhausted) {
      for (int c = lane; c < N * k; c += 64) {
        const int n = c / k, j = c - n * k;
        const float v = base[(int64_t)n * W + 3 + j];
        const int id = __float_as_int(base[(int64_t)n * W + 3 + k + j]);
        if (id >= 0 && plp_behind(v, id, pv, pi) && plp_ahead(v, id, bv, bi)) { bv = v; bi = id; }
      }
      plp_wave_best(bv, bi);
    }
    if (bi == PLP_NONE) exhausted = true;
    if (lane == 0) {
      const float v = exhausted ? -INFINITY : bv;
      const int id = exhausted ? -1 : bi;
      if (out_rec != nullptr) {
        out_rec[(int64_t)r * W + 3 + q] = v;
        out_rec[(int64_t)r * W + 3 + k + q] = __int_as_float(id);
      } else {
        top_lp[(int64_t)r * k + q] = exhausted ? -INFINITY : lp(v);
        top_id[(int64_t)r * k + q] = id;
      }
    }
    pv = bv;
    pi = bi;
  }
}

// Workgroups per row: the slices must fit the LDS stage; at small R enough workgroups to
// cover the chip, as K10's sample_splits does.
int plp_splits(int R, int ncols) {
  const int need = std::max(1, (ncols + PLP_CAP - 1) / PLP_CAP);
  const int want = R >= 512 ? 1 : std::min(32, (512 + R - 1) / std::max(R, 1));
  return std::max(need, want);
}

int plp_cap() { return PLP_CAP; }

void launch_plp_partial(int dtype, float* rec, const void* logits, int64_t row_stride,
                        const int64_t* targets, int R, int S, int vocab_off, int ncols, int k,
                        hipStream_t s) {
  if (R == 0) return;
  const dim3 grid(R, S);
  if (dtype == DT_BF16)
    plp_partial_kernel<bf16><<<grid, PLP_NT, 0, s>>>(rec, (const bf16*)logits, row_stride, targets,
                                                     vocab_off, ncols, k);
  else if (dtype == DT_F16)
    plp_partial_kernel<f16><<<grid, PLP_NT, 0, s>>>(rec, (const f16*)logits, row_stride, targets,
                                                    vocab_off, ncols, k);
  else
    plp_partial_kernel<float><<<grid, PLP_NT, 0, s>>>(rec, (const float*)logits, row_stride,
                                                      targets, vocab_off, ncols, k);
}

void launch_plp_merge(float* tok_lp, float* top_lp, int* top_id, float* out_rec, const float* rec,
                      int R, int N, int k, hipStream_t s) {
  if (R == 0) return;
  plp_merge_kernel<<<R, 64, 0, s>>>(tok_lp, top_lp, top_id, out_rec, rec, N, k);
}

}  // namespace kgc
