// K9a: W8A8 GEMM for gfx950 -- e4m3 activations x e4m3 weights on the fp8 MFMA, for the
// prefill / mixed / untuned M > 64 linears of a --quantization fp8_w8a8 model:
//
//   act_quant_fp8:  xs[m] = amax(|x[m, :]|) / 448 (1 for an all-zero row),
//                   xq[m, k] = e4m3(clamp(x[m, k] / xs[m], +-448))           (per-token, online)
//   w8a8_gemm:      C[m, n] = (sum_k xq[m, k] * w8[n, k]) * xs[m] * ws[n] (+ bias[n])
//
// The GEMM.  K9m's skeleton (gemm_decode.hip): 512-thread workgroups, 4 (M) x 2 (N) waves,
// both operands HBM/L2 -> LDS by 16-byte LDS-DMA into a ring retired by counted
// `s_waitcnt vmcnt(N)` + a raw s_barrier, the weight stream non-temporal (aux = 2).  What
// is K9a's own:
//   * Both operands are one byte per element, so a K-step is BK = 128 k: a 128-byte LDS row
//     for A and for B alike, and v_mfma_f32_16x16x128_f8f6f4 (cbsz = blgp = 0: e4m3 x e4m3,
//     scales x1) consumes a whole step per instruction.  No conversion instruction anywhere.
//   * The weight is read IN PLACE, row-major e4m3 [N, K] as quantize_model made it: no
//     packed copy.  A 1-KiB DMA piece is 8 tile rows (8 x 128 B, rows K bytes apart), for
//     both operands; lane l of a piece fills LDS row 8p + l / 8, chunk position l % 8, with
//     global 16-B chunk (l % 8) ^ (row % 8) -- K9m's swizzle, applied on the source address.
//   * Fragment mapping.  Lane (r = lane % 16, q = lane / 16) feeds the MFMA eight registers
//     (32 bytes) per operand; it loads them as TWO ds_read_b128: chunk q (row bytes
//     16 q + [0, 16)) into registers 0-3 and chunk 4 + q (bytes 64 + 16 q + [0, 16)) into
//     registers 4-7, for A and for B alike.  Whatever k the instruction assigns to byte j
//     of lane group q, A and B put the same k there, and the four groups' chunks
//     {q, 4 + q} cover all 128 bytes of the row once: the contraction is over the whole
//     step.  (The natural "bytes 32 q + [0, 32)" mapping would read chunks 2 q and 2 q + 1:
//     in a 16-lane service group the lanes with q = 0 and q = 1 then land on the same
//     parity of chunk position and collide two ways.)
//   * Bank argument for these reads: with chunks {q, 4 + q} each ds_read_b128 is exactly
//     K9m's read of k-sub-step ks = 0 / 1 (chunk 4 ks + fq of row fr, at position
//     chunk ^ (row % 8)); a wave's row base is a multiple of 16, so row % 8 = fr % 8.  A
//     b128 read is served in four 16-lane groups, conflict-free iff the 16 lanes touch 16
//     distinct 16-B slots of the 256-B bank row; slot(r, p) = 8 (r % 2) + p.  Group 0 is
//     q = 0 with fr in {0-3, 12-15} and q = 1 with fr in {4-11}: j = fr % 8 takes every
//     value once per q, positions are c ^ j with c = 4 ks + q.  Within one q the eight
//     positions are distinct.  Across q = 0 / 1: equal slots need equal row parity and
//     equal position, c0 ^ j0 = c1 ^ j1 with c0 ^ c1 = 1, so j0 ^ j1 = 1 -- opposite
//     parity.  Distinct.  Group 1 swaps the two fr sets; groups 2 and 3 are q = 2 / 3, where
//     c0 ^ c1 = 1 again.
//   * Tiles 256 x 128 (3-slot ring, 3 x 48 KB), 256 x 256 (2 slots, 2 x 64 KB: plain double
//     buffering) and 128 x 128 (3 or 4 slots of 32 KB) against the 160 KiB of LDS.  The
//     256-row tiles stay on the 16x16x128 form (one instruction per K-step and 16 x 16
//     output tile, the fragment reads above proven conflict-free); the 32x32x64 form was
//     not built and not measured.
//   * Row blocks are walked in bands of 8 with the row block fastest, so the 8 XCDs
//     (workgroup j runs on XCD j % 8) each keep ONE activation row block in their L2 while
//     the column tiles' weights stream past.
//   * Every configuration walks K from 0 up in whole steps, one accumulator per output,
//     no split-K: all configurations return the same bits.
//   * Ragged edges: rows >= M re-read row M - 1 and are never stored; N is a multiple of
//     128, so a 256-column tile may hang over by 128: those weight rows re-read row N - 1
//     and their columns are never stored.
//   * Epilogue: acc * xs[m] * ws[n] in fp32, + bias[n], one rounding to bf16 / f16.
//
// The quantiser.  One wave per row: a lane holds 16 consecutive elements (two 16-byte
// loads) of each 1024-element span of the row, the whole row stays in registers (K <=
// 16384: 16 spans) between the amax pass and the convert pass, and the lane writes its 16
// e4m3 as one 16-byte store.  Division is IEEE fp32 (__fdiv_rn), the clamp precedes the
// conversion, rounding is common.h fp8x4's (nearest-even): the result is
// ops/quant.py quantize_fp8_rows bit for bit.  Work split: up to 1024 rows, one-wave
// workgroups, one per row (300 rows put a wave on every one of the 256 CUs); above that,
// 4-wave workgroups, at most 2048 of them, each wave striding over rows (16384 rows:
// 2048 workgroups x 4 waves x 2 rows).
//
// Resource report: at the configuration table below.
#include "common.h"
#include "launch.h"

namespace kgc {

namespace {

constexpr int AG_THREADS = 512;     // 8 waves: 4 along M x 2 along N
constexpr int AG_BK = 128;          // k per step = bytes per LDS row, both operands

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void gbl_void;

template <int AUX>
__device__ __forceinline__ void glds16(const void* src, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((gbl_void*)src, (lds_void*)lds_wave_base, 16, 0, AUX);
}

template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// wait until at most min(D, younger) steps of L DMAs each are still in flight
template <int L, int D>
__device__ __forceinline__ void wait_younger(int younger) {
  if constexpr (D > 0) if (younger >= D) { wait_vm<D * L>(); return; }
  if constexpr (D > 1) if (younger == 1) { wait_vm<L>(); return; }
  wait_vm<0>();
}

template <typename T, int BM, int BN, int NS>
__global__ __launch_bounds__(AG_THREADS, 1) void w8a8_gemm_kernel(
    T* __restrict__ C, const uint8_t* __restrict__ Xq, const float* __restrict__ xs,
    const uint8_t* __restrict__ W, const float* __restrict__ ws, const T* __restrict__ bias,
    int M, int N, int K, int64_t ldc, int MB, int NB) {
  constexpr int MT = BM / 4 / 16;                 // 16-row MFMA tiles per wave
  constexpr int NT = BN / 2 / 16;                 // 16-col MFMA tiles per wave
  constexpr int LA = BM / 64, LB = BN / 64;       // 1-KiB pieces per wave per step
  constexpr int L = LA + LB;
  constexpr int A_BYTES = BM * AG_BK, SLOT_BYTES = A_BYTES + BN * AG_BK;
  static_assert(NS >= 2 && NS <= 4 && NS * SLOT_BYTES <= 163840, "LDS ring: 2..4 slots, 160 KiB");
  static_assert((NS - 2) * L <= 63, "vmcnt is 6 bits");
  __shared__ __attribute__((aligned(16))) char lds[NS * SLOT_BYTES];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  // bands of 8 row blocks, row block fastest (the last band may be shorter)
  const int band = blockIdx.x / (8 * NB);
  const int in_band = blockIdx.x - band * (8 * NB);
  const int rows_in_band = MB - band * 8 < 8 ? MB - band * 8 : 8;
  const int mb = band * 8 + in_band % rows_in_band, nb = in_band / rows_in_band;
  const int m0 = mb * BM, n0 = nb * BN;

  // ---- DMA sources: lane l of piece p fills LDS row 8p + l/8, position l%8 with global
  // chunk (l%8) ^ (row%8), for both operands
  const int drow = lane >> 3, dchunk = (lane & 7) ^ drow;
  const uint8_t* a_src[LA];
  const uint8_t* b_src[LB];
#pragma unroll
  for (int t = 0; t < LA; ++t) {
    int r = m0 + (wave * LA + t) * 8 + drow;
    r = r < M ? r : M - 1;                        // padded rows re-read the last row
    a_src[t] = Xq + (int64_t)r * K + dchunk * 16;
  }
#pragma unroll
  for (int t = 0; t < LB; ++t) {
    int r = n0 + (wave * LB + t) * 8 + drow;
    r = r < N ? r : N - 1;                        // a 256-column tile over the edge of N
    b_src[t] = W + (int64_t)r * K + dchunk * 16;
  }
  const int nk = K / AG_BK;

  auto issue = [&](int slot, int step) {
    char* sa = lds + slot * SLOT_BYTES;
    char* sb = sa + A_BYTES;
    const int64_t ko = (int64_t)step * AG_BK;
#pragma unroll
    for (int t = 0; t < LA; ++t) glds16<0>(a_src[t] + ko, sa + (wave * LA + t) * 1024);
#pragma unroll
    for (int t = 0; t < LB; ++t) glds16<2>(b_src[t] + ko, sb + (wave * LB + t) * 1024);
  };

  f32x4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[i][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fq = lane >> 4;
  const int a_row0 = wm * (BM / 4) + fr;
  const int b_row0 = wn * (BN / 2) + fr;
  // the lane's channel scales, loaded before the K walk hides their latency; they are
  // older than every DMA, so the counted waits below cover them.  (The optional bias is
  // loaded in the epilogue: a conditional load here would wait for itself before the ring
  // starts.)
  float sc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    int col = n0 + b_row0 + n * 16;
    col = col < N ? col : N - 1;
    sc[n] = ws[col];
  }

  // NS-slot ring: NS - 1 steps issued ahead, NS - 2 of them in flight behind the one read
#pragma unroll
  for (int p = 0; p < NS - 1; ++p)
    if (p < nk) issue(p, p);
  int slot = 0;
  for (int it = 0; it < nk; ++it) {
    wait_younger<L, NS - 2>(nk - 1 - it);
    __builtin_amdgcn_s_barrier();
    // the slot read in iteration it - 1 (every wave has passed the barrier since)
    if (it + NS - 1 < nk) issue(slot == 0 ? NS - 1 : slot - 1, it + NS - 1);
    const char* sa = lds + slot * SLOT_BYTES;
    const char* sb = sa + A_BYTES;
    slot = slot == NS - 1 ? 0 : slot + 1;
    // chunks fq and 4 + fq of the lane's row, each at position chunk ^ (row % 8)
    i32x8 af[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int r = a_row0 + i * 16;
      const u32x4 lo = *reinterpret_cast<const u32x4*>(sa + r * AG_BK + ((fq ^ (r & 7)) << 4));
      const u32x4 hi = *reinterpret_cast<const u32x4*>(sa + r * AG_BK + (((4 + fq) ^ (r & 7)) << 4));
      af[i] = i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w,
                    (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
    }
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int r = b_row0 + n * 16;
      const u32x4 lo = *reinterpret_cast<const u32x4*>(sb + r * AG_BK + ((fq ^ (r & 7)) << 4));
      const u32x4 hi = *reinterpret_cast<const u32x4*>(sb + r * AG_BK + (((4 + fq) ^ (r & 7)) << 4));
      const i32x8 bf = i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w,
                             (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
#pragma unroll
      for (int i = 0; i < MT; ++i)
        acc[i][n] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af[i], bf, acc[i][n], 0, 0,
                                                                     0, 0, 0, 0);
    }
  }

  // ---- epilogue: lane holds C[4*fq + e][fr] of every 16x16 tile
  float bv[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    asm volatile("" : "+v"(sc[n]));
    int col = n0 + b_row0 + n * 16;
    col = col < N ? col : N - 1;
    bv[n] = bias != nullptr ? to_f<T>(bias[col]) : 0.f;
  }
#pragma unroll
  for (int i = 0; i < MT; ++i) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int row = m0 + wm * (BM / 4) + i * 16 + fq * 4 + e;
      if (row >= M) continue;
      const float xr = xs[row];
      T* cp = C + (int64_t)row * ldc + n0 + wn * (BN / 2) + fr;
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        if (BN > 128 && n0 + wn * (BN / 2) + n * 16 >= N) continue;
        cp[n * 16] = from_f<T>(acc[i][n][e] * xr * sc[n] + bv[n]);
      }
    }
  }
}

// Tile table: id -> (BM, BN, ring slots).  Resource report (hipcc
// -Rpass-analysis=kernel-resource-usage, gfx950; bf16 and f16 alike, AGPRs 0, scratch 0,
// no spills everywhere; 2 waves per SIMD = the one 512-thread workgroup per CU):
//   256 x 128, 3 slots (144 KB)   150 VGPRs
//   256 x 256, 2 slots (128 KB)   229 VGPRs
//   128 x 128, 4 slots (128 KB)    98 VGPRs
//   128 x 128, 3 slots ( 96 KB)    96 VGPRs
// act_quant_fp8, 1 / 2 / 4 / 8 / 16 spans: 37 / 45 / 61 / 93 / 157 VGPRs, no scratch.
struct AgCfg {
  int bm, bn, ns;
};
constexpr int kNumCfgs = 4;
static const AgCfg kCfg[kNumCfgs] = {{256, 128, 3}, {256, 256, 2}, {128, 128, 4}, {128, 128, 3}};

template <typename T, int BM, int BN, int NS>
void w8a8_gemm_cfg(void* C, const void* Xq, const float* xs, const void* W, const float* ws,
                   const void* bias, int M, int N, int K, int64_t ldc, hipStream_t s) {
  const int MB = (M + BM - 1) / BM, NB = (N + BN - 1) / BN;
  w8a8_gemm_kernel<T, BM, BN, NS><<<dim3((unsigned)(MB * NB)), AG_THREADS, 0, s>>>(
      (T*)C, (const uint8_t*)Xq, xs, (const uint8_t*)W, ws, (const T*)bias, M, N, K, ldc, MB, NB);
}

template <typename T>
void w8a8_gemm_t(int cfg, void* C, const void* Xq, const float* xs, const void* W,
                 const float* ws, const void* bias, int M, int N, int K, int64_t ldc,
                 hipStream_t s) {
  switch (cfg) {
    case 0: w8a8_gemm_cfg<T, 256, 128, 3>(C, Xq, xs, W, ws, bias, M, N, K, ldc, s); break;
    case 1: w8a8_gemm_cfg<T, 256, 256, 2>(C, Xq, xs, W, ws, bias, M, N, K, ldc, s); break;
    case 2: w8a8_gemm_cfg<T, 128, 128, 4>(C, Xq, xs, W, ws, bias, M, N, K, ldc, s); break;
    case 3: w8a8_gemm_cfg<T, 128, 128, 3>(C, Xq, xs, W, ws, bias, M, N, K, ldc, s); break;
    default: break;                 // the host checks cfg < w8a8_gemm_num_cfgs()
  }
}

// ---- the quantiser: one wave per row, R spans of 1024 elements held in registers
constexpr int AQ_MAX_SPANS = 16;

template <typename T, int R>
__global__ __launch_bounds__(256) void act_quant_fp8_kernel(uint8_t* __restrict__ Xq,
                                                            float* __restrict__ xs,
                                                            const T* __restrict__ X, int M, int K,
                                                            int64_t ldx) {
  const int lane = threadIdx.x & 63;
  const int waves = blockDim.x >> 6;
  const int stride = gridDim.x * waves;
  for (int row = blockIdx.x * waves + (threadIdx.x >> 6); row < M; row += stride) {
    const T* xr = X + (int64_t)row * ldx;
    Pack8<T> v[R][2];
    float amax = 0.f;
#pragma unroll
    for (int s = 0; s < R; ++s) {
      const int k = (s * 64 + lane) * 16;
      if (k < K) {
        v[s][0].u = *reinterpret_cast<const u32x4*>(xr + k);
        v[s][1].u = *reinterpret_cast<const u32x4*>(xr + k + 8);
      } else {
        v[s][0].u = v[s][1].u = u32x4{0u, 0u, 0u, 0u};
      }
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(to_f<T>(v[s][h].h[j])));
    }
    amax = wave_max(amax);
    const float scale = amax > 0.f ? __fdiv_rn(amax, FP8_MAX) : 1.f;
    if (lane == 0) xs[row] = scale;
#pragma unroll
    for (int s = 0; s < R; ++s) {
      const int k = (s * 64 + lane) * 16;
      if (k >= K) continue;
      float f[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) f[j] = __fdiv_rn(to_f<T>(v[s][j >> 3].h[j & 7]), scale);
      *reinterpret_cast<u32x4*>(Xq + (int64_t)row * K + k) =
          u32x4{fp8x4(f[0], f[1], f[2], f[3]), fp8x4(f[4], f[5], f[6], f[7]),
                fp8x4(f[8], f[9], f[10], f[11]), fp8x4(f[12], f[13], f[14], f[15])};
    }
  }
}

template <typename T, int R>
void act_quant_fp8_r(void* Xq, float* xs, const void* X, int M, int K, int64_t ldx,
                     hipStream_t s) {
  // up to 1024 rows: a one-wave workgroup per row; above: 4 waves, at most 2048 workgroups
  const bool small = M <= 1024;
  const int grid = small ? M : ((M + 3) / 4 < 2048 ? (M + 3) / 4 : 2048);
  act_quant_fp8_kernel<T, R><<<dim3((unsigned)grid), small ? 64 : 256, 0, s>>>(
      (uint8_t*)Xq, xs, (const T*)X, M, K, ldx);
}

template <typename T>
void act_quant_fp8_t(void* Xq, float* xs, const void* X, int M, int K, int64_t ldx,
                     hipStream_t s) {
  const int spans = (K + 1023) / 1024;
  if (spans <= 1) act_quant_fp8_r<T, 1>(Xq, xs, X, M, K, ldx, s);
  else if (spans <= 2) act_quant_fp8_r<T, 2>(Xq, xs, X, M, K, ldx, s);
  else if (spans <= 4) act_quant_fp8_r<T, 4>(Xq, xs, X, M, K, ldx, s);
  else if (spans <= 8) act_quant_fp8_r<T, 8>(Xq, xs, X, M, K, ldx, s);
  else act_quant_fp8_r<T, AQ_MAX_SPANS>(Xq, xs, X, M, K, ldx, s);
}

}  // namespace

int w8a8_gemm_num_cfgs() { return kNumCfgs; }
void w8a8_gemm_cfg_info(int cfg, int* bm, int* bn, int* ns) {
  *bm = kCfg[cfg].bm;
  *bn = kCfg[cfg].bn;
  *ns = kCfg[cfg].ns;
}
int act_quant_fp8_max_k() { return AQ_MAX_SPANS * 1024; }

void launch_w8a8_gemm(int dtype, int cfg, void* C, const void* Xq, const float* xs,
                      const void* W8, const float* ws, const void* bias, int M, int N, int K,
                      int64_t ldc, hipStream_t s) {
  if (dtype == DT_BF16) w8a8_gemm_t<bf16>(cfg, C, Xq, xs, W8, ws, bias, M, N, K, ldc, s);
  else w8a8_gemm_t<f16>(cfg, C, Xq, xs, W8, ws, bias, M, N, K, ldc, s);
}

void launch_act_quant_fp8(int dtype, void* Xq, float* xs, const void* X, int M, int K,
                          int64_t ldx, hipStream_t s) {
  if (M == 0) return;
  if (dtype == DT_BF16) act_quant_fp8_t<bf16>(Xq, xs, X, M, K, ldx, s);
  else act_quant_fp8_t<f16>(Xq, xs, X, M, K, ldx, s);
}

}  // namespace kgc
