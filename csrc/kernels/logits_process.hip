// K16 logits processing: presence / frequency / repetition penalties, logit_bias and min_p,
// in place on the rows of logits [S, >= V] that a per-step table names, plus the two small
// kernels that keep the per-slot token statistics.
//
// Statistics: one uint32 word per (slot, token), stats [slots, V].  Bit 31: the token is in
// the prompt; low 31 bits: how often it was generated.  word != 0 <=> "seen".
//
// Table (one int32 block per step, floats as their bits; R rows, nb bias entries):
//   row[R] slot[R] pres[R] freq[R] rep[R] min_p[R] t[R] off[R + 1] ids[nb] vals[nb]
// row: the logits row; slot: its statistics row, -1 for a row without penalties; off: CSR
// offsets of the row's logit_bias entries.  The kernels trust nothing in it: a row or slot
// out of range skips the table row, offsets are clamped to [0, nb], ids outside the slice
// (so also ids >= V) are ignored.
//
// lp_apply_kernel, grid (slices, R), 256 threads: slice y of table row j is the columns
// [y * chunk, min(V, (y + 1) * chunk)), chunk <= LP_CAP.  The workgroup
//   1. reads its slice from HBM once with 16-byte loads for every dtype (the unaligned head
//      and the tail as scalars, so rows at any element offset and stride take the vector
//      path) and stages it in LDS as fp32;
//   2. reads the same columns of the slot's statistics row with 16-byte loads (its own head
//      and tail: the two rows are misaligned independently) and, for non-zero words only,
//      rewrites the staged value: s > 0 ? s / rep : s * rep, then - freq * count
//      - pres * (count > 0).  Each column belongs to one thread here, so no atomics;
//   3. wave 0 scans the row's bias entries 64 at a time and applies those inside the slice
//      with LDS float atomic adds, ONE lane at a time in entry order: duplicates accumulate,
//      and the sum is the same bits in both passes (pass B must reproduce pass A's values);
//   4. min_p: keep s iff s >= smax + t * ln(min_p) -- softmax(s / t) >= min_p * max softmax
//      with the normalising sum cancelled, so no row sum.  smax needs the whole processed
//      row: rows with min_p take pass A (steps 1-3, then only the slice maximum goes to
//      pmax[j][y]) and pass B (steps 1-3 again, max over pmax[j][*], threshold, store);
//      rows without take pass B alone.  An all -inf row has smax = -inf and stays -inf;
//   5. stores the slice with the staging pattern mirrored, one rounding to the dtype.
//      Untouched columns round-trip dtype -> fp32 -> dtype, which is the identity.
// Columns >= V are never read or written.  -inf stays -inf under every rule (rep > 0).
//
// lp_update_kernel: stats[slot[j]][clamp(sampled[row[j]])] += 1 for table rows with a slot.
// lp_init_kernel: after a memset of the slot's row, OR bit 31 for the first n_prompt tokens
// of a list and add 1 for the rest (ids outside [0, V) ignored).
//
// hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage:
//   lp_apply_kernel<bf16 / f16> pass A  18 VGPR  54 SGPR  LDS 32800 B  scratch 0  4 waves/SIMD
//   lp_apply_kernel<bf16 / f16> pass B  26 VGPR  66 SGPR  LDS 32800 B  scratch 0  4 waves/SIMD
//   lp_apply_kernel<float> pass A       16 VGPR  53 SGPR  LDS 32800 B  scratch 0  4 waves/SIMD
//   lp_apply_kernel<float> pass B       20 VGPR  64 SGPR  LDS 32800 B  scratch 0  4 waves/SIMD
//   lp_update_kernel                     8 VGPR  14 SGPR  LDS     0 B  scratch 0  8 waves/SIMD
//   lp_init_kernel                       4 VGPR  14 SGPR  LDS     0 B  scratch 0  8 waves/SIMD
// (4 workgroups of 4 waves per CU, bounded by the LDS stage)
#include "common.h"
#include "launch.h"
#include <algorithm>

namespace kgc {

constexpr int LP_NT = 256;
constexpr int LP_CAP = 8192;                 // columns a workgroup stages (32 KB of LDS as fp32)
constexpr uint32_t LP_PROMPT = 0x80000000u;  // statistics word: "in the prompt"

struct LpTable {
  const int *row, *slot;
  const float *pres, *freq, *rep, *minp, *temp;
  const int *off, *ids;
  const float* vals;
};
__device__ __forceinline__ LpTable lp_table(const int* tab, int R, int nb) {
  const float* f = reinterpret_cast<const float*>(tab);
  const int64_t r = R;
  return LpTable{tab,       tab + r,       f + 2 * r,         f + 3 * r,          f + 4 * r,
                 f + 5 * r, f + 6 * r,     tab + 7 * r,       tab + 8 * r + 1,    f + 8 * r + 1 + nb};
}

template <typename T, bool PASS_A>
__global__ __launch_bounds__(LP_NT) void lp_apply_kernel(
    T* __restrict__ logits, int64_t row_stride, int S, const uint32_t* __restrict__ stats,
    int nslots, const int* __restrict__ tab, int R, int nb, int V, int chunk,
    float* __restrict__ pmax) {
  constexpr int EPV = 16 / (int)sizeof(T);           // elements per 16-byte vector
  __shared__ __attribute__((aligned(16))) float x[LP_CAP + 4];
  __shared__ float red[LP_NT / 64];
  const int y = blockIdx.x, j = blockIdx.y, nsl = gridDim.x, tid = threadIdx.x;
  const LpTable t = lp_table(tab, R, nb);
  const float minp = t.minp[j];
  const bool mp = minp > 0.f;
  if (PASS_A && !mp) return;
  const int r = t.row[j];
  const int lo = y * chunk;
  const int len = min(min(chunk, LP_CAP), V - lo);
  if (r < 0 || r >= S || len <= 0) return;            // (block-uniform)
  T* src = logits + (int64_t)r * row_stride + lo;

  // ---- 1. HBM -> LDS.  The staged copy starts at x[pad] so that every 16-byte vector of
  // the row lands 16-byte aligned in LDS too
  const int mis = (int)(reinterpret_cast<uintptr_t>(src) & 15) / (int)sizeof(T);
  const int head = min(len, (EPV - mis) % EPV);
  const int nvec = (len - head) / EPV;
  const int pad = (4 - (head & 3)) & 3;
  float* xs = x + pad;
  if (tid < head) xs[tid] = to_f(src[tid]);
  for (int v = tid; v < nvec; v += LP_NT) {
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
  for (int i = head + nvec * EPV + tid; i < len; i += LP_NT) xs[i] = to_f(src[i]);
  __syncthreads();

  // ---- 2. penalties from the statistics words of the same columns
  const int slot = t.slot[j];
  if (stats != nullptr && slot >= 0 && slot < nslots) {
    const float pres = t.pres[j], freq = t.freq[j], rep = t.rep[j];
    const uint32_t* sp = stats + (int64_t)slot * V + lo;
    auto touch = [&](int c, uint32_t w) {
      if (w == 0u) return;
      const float cnt = (float)(w & ~LP_PROMPT);
      float s = xs[c];
      s = s > 0.f ? __fdiv_rn(s, rep) : s * rep;
      xs[c] = s - freq * cnt - (cnt > 0.f ? pres : 0.f);
    };
    const int shead = min(len, (4 - (int)((reinterpret_cast<uintptr_t>(sp) & 15) >> 2)) & 3);
    const int snvec = (len - shead) >> 2;
    if (tid < shead) touch(tid, sp[tid]);
    for (int v = tid; v < snvec; v += LP_NT) {
      const int c = shead + 4 * v;
      const u32x4 w = *reinterpret_cast<const u32x4*>(sp + c);
      if ((w.x | w.y | w.z | w.w) != 0u) {
        touch(c, w.x);
        touch(c + 1, w.y);
        touch(c + 2, w.z);
        touch(c + 3, w.w);
      }
    }
    for (int i = shead + 4 * snvec + tid; i < len; i += LP_NT) touch(i, sp[i]);
  }
  __syncthreads();

  // ---- 3. logit_bias: wave 0, 64 entries a round, the lanes inside the slice one by one
  if (tid < 64) {
    const int e0 = min(max(t.off[j], 0), nb), e1 = min(max(t.off[j + 1], e0), nb);
    for (int base = e0; base < e1; base += 64) {
      const int e = base + tid;
      int c = -1;
      float val = 0.f;
      if (e < e1) {
        const int id = t.ids[e];
        if (id >= lo && id < lo + len) {
          c = id - lo;
          val = t.vals[e];
        }
      }
      unsigned long long m = __ballot(c >= 0);
      while (m != 0ull) {
        if (tid == __ffsll(m) - 1) atomicAdd(&xs[c], val);
        m &= m - 1ull;
      }
    }
  }
  __syncthreads();

  // ---- 4. min_p
  if constexpr (PASS_A) {
    float m = -INFINITY;
    for (int i = tid; i < len; i += LP_NT) m = fmaxf(m, xs[i]);
    m = block_max<LP_NT>(m, red);
    if (tid == 0) pmax[(int64_t)j * nsl + y] = m;
  } else {
  float thr = -INFINITY;
  if (mp) {
    float m = -INFINITY;
    for (int n = tid; n < nsl; n += LP_NT) m = fmaxf(m, pmax[(int64_t)j * nsl + n]);
    m = block_max<LP_NT>(m, red);
    thr = m + t.temp[j] * logf(minp);
  }
  // (!mp: every value, a NaN included, goes back as it is)
  auto fin = [&](float s) { return (mp && !(s >= thr)) ? -INFINITY : s; };

  // ---- 5. LDS -> HBM, the staging pattern mirrored
  if (tid < head) src[tid] = from_f<T>(fin(xs[tid]));
  for (int v = tid; v < nvec; v += LP_NT) {
    const float* d = xs + head + v * EPV;
    const f32x4 a = *reinterpret_cast<const f32x4*>(d);
    if constexpr (sizeof(T) == 2) {
      const f32x4 b = *reinterpret_cast<const f32x4*>(d + 4);
      Pack8<T> p;
      p.h[0] = from_f<T>(fin(a.x));
      p.h[1] = from_f<T>(fin(a.y));
      p.h[2] = from_f<T>(fin(a.z));
      p.h[3] = from_f<T>(fin(a.w));
      p.h[4] = from_f<T>(fin(b.x));
      p.h[5] = from_f<T>(fin(b.y));
      p.h[6] = from_f<T>(fin(b.z));
      p.h[7] = from_f<T>(fin(b.w));
      *reinterpret_cast<u32x4*>(src + head + v * EPV) = p.u;
    } else {
      *reinterpret_cast<f32x4*>(src + head + v * EPV) = f32x4{fin(a.x), fin(a.y), fin(a.z), fin(a.w)};
    }
  }
  for (int i = head + nvec * EPV + tid; i < len; i += LP_NT) src[i] = from_f<T>(fin(xs[i]));
  }
}

__global__ __launch_bounds__(LP_NT) void lp_update_kernel(
    uint32_t* __restrict__ stats, int nslots, const int* __restrict__ tab, int R,
    const int64_t* __restrict__ sampled, int S, int V) {
  const int j = blockIdx.x * LP_NT + threadIdx.x;
  if (j >= R) return;
  const int row = tab[j], slot = tab[(int64_t)R + j];
  if (row < 0 || row >= S || slot < 0 || slot >= nslots) return;
  const int64_t tok = min(max(sampled[row], (int64_t)0), (int64_t)V - 1);
  atomicAdd(&stats[(int64_t)slot * V + tok], 1u);
}

__global__ __launch_bounds__(LP_NT) void lp_init_kernel(
    uint32_t* __restrict__ srow, const int* __restrict__ toks, int n, int n_prompt, int V) {
  const int i = blockIdx.x * LP_NT + threadIdx.x;
  if (i >= n) return;
  const int tok = toks[i];
  if (tok < 0 || tok >= V) return;
  if (i < n_prompt)
    atomicOr(&srow[tok], LP_PROMPT);
  else
    atomicAdd(&srow[tok], 1u);
}

int lp_cap() { return LP_CAP; }

// Columns per workgroup: the LDS stage at most; fewer when R rows of LP_CAP-column slices
// would leave most of the chip idle (about two workgroups per CU is the aim).
int lp_chunk(int R, int V) {
  int c = LP_CAP;
  while (c > 1024 && (int64_t)std::max(R, 1) * ((V + c - 1) / c) < 512) c >>= 1;
  return c;
}

void launch_lp_apply(int dtype, void* logits, int64_t row_stride, int S, const uint32_t* stats,
                     int nslots, const int* tab, int R, int nb, int V, int chunk, bool any_minp,
                     float* pmax, hipStream_t s) {
  if (R == 0 || V == 0) return;
  const dim3 grid((V + chunk - 1) / chunk, R);
#define KGC_LP_LAUNCH(T, A)                                                                      \
  lp_apply_kernel<T, A><<<grid, LP_NT, 0, s>>>((T*)logits, row_stride, S, stats, nslots, tab, R, \
                                               nb, V, chunk, pmax)
  for (int pass = any_minp ? 0 : 1; pass < 2; ++pass) {
    if (dtype == DT_BF16) {
      if (pass == 0) KGC_LP_LAUNCH(bf16, true); else KGC_LP_LAUNCH(bf16, false);
    } else if (dtype == DT_F16) {
      if (pass == 0) KGC_LP_LAUNCH(f16, true); else KGC_LP_LAUNCH(f16, false);
    } else {
      if (pass == 0) KGC_LP_LAUNCH(float, true); else KGC_LP_LAUNCH(float, false);
    }
  }
#undef KGC_LP_LAUNCH
}

void launch_lp_update(uint32_t* stats, int nslots, const int* tab, int R, const int64_t* sampled,
                      int S, int V, hipStream_t s) {
  if (R == 0) return;
  lp_update_kernel<<<(R + LP_NT - 1) / LP_NT, LP_NT, 0, s>>>(stats, nslots, tab, R, sampled, S, V);
}

void launch_lp_init(uint32_t* srow, const int* toks, int n, int n_prompt, int V, hipStream_t s) {
  (void)hipMemsetAsync(srow, 0, (size_t)V * sizeof(uint32_t), s);
  if (n == 0) return;
  lp_init_kernel<<<(n + LP_NT - 1) / LP_NT, LP_NT, 0, s>>>(srow, toks, n, n_prompt, V);
}

}  // namespace kgc
