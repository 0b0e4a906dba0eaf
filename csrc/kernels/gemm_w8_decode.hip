// K9mq: the K9m mid-batch decode pipeline (gemm_decode.hip) over weight-only FP8 (W8A16)
// weights, for the decode buckets with 64 < M <= 512 of a --quantization fp8 model:
//
//   C[M, N] = (X[M, K] . W8[N, K]^T) * scale[N]      X / C bf16 or f16, W8 OCP e4m3,
//                                                    one fp32 scale per output row
//
// The structure is K9m's: 512-thread workgroups (4 (M) x 2 (N) waves of
// v_mfma_f32_16x16x32), both operands HBM/L2 -> LDS by 16-byte LDS-DMA into a ring retired
// by counted `s_waitcnt vmcnt(N)` + a raw s_barrier, the weight stream non-temporal
// (aux = 2), each workgroup's K walk rotated, split-K over a 1-D grid with z = L % S.
// The activation operand is K9m's to the byte: 128-B LDS rows, 16-B chunk c of row r at
// chunk position c ^ (r % 8), the XOR applied on the DMA source address and on the read.
// What differs is the weight operand, which stays e4m3 in LDS:
//   * a 64-k step of a weight row is 64 bytes, so a 256 x 128 slot is 32 + 8 = 40 KB (a
//     4-slot ring fits the 160 KiB) and a 1-KiB DMA piece is 16 tile rows;
//   * PACKED weights only (w8_dgemm_pack): tiles [N/128][K/64][128 rows x 64 B], one
//     contiguous 8 KB block per K-step of a column tile, streamed lane-linear.  Inside a
//     64-byte row the pack puts 16-byte chunk q = k in 8q + [0, 8) followed by k in
//     32 + 8q + [0, 8): lane (r16, q4) reads ONE ds_read_b128 and widens it (common.h
//     fp8x8_widen, exact) into its B fragments of BOTH MFMAs of the step in the standard
//     k order, so the activation fragments are read exactly as K9m reads them;
//   * chunk q of tile row r sits at chunk position q ^ g((r / 4) % 4), g = (0, 2, 3, 1),
//     baked into the packed tiles (the DMA copies them linearly) and applied on the read.
//     Bank argument: a ds_read_b128 is served in four 16-lane groups, each conflict-free
//     iff its 16 lanes touch 16 distinct 16-B slots of the 256-B bank row; the slot of
//     (r, position p) is 4 (r % 4) + p.  Group 0 is lanes {0-3, 12-15} (q = 0, rows 0-3
//     and 12-15 of the wave's 16) and {20-27} (q = 1, rows 4-11).  The four rows with one
//     value of r % 4 are j = r / 4 = 0, 3 (q = 0) and 1, 2 (q = 1): positions g(0), g(3),
//     1 ^ g(1), 1 ^ g(2) = 0, 1, 3, 2 -- distinct.  Group 1 ({4-11}: q = 0, j = 1, 2;
//     {16-19, 28-31}: q = 1, j = 0, 3): g(1), g(2), 1 ^ g(0), 1 ^ g(3) = 2, 3, 1, 0.
//     Groups 2 and 3 are groups 0 and 1 with q + 2: the same sets XOR 2.  (Unswizzled, the
//     four rows of a group with one r % 4 share a position: 4-way; the plain XOR with j is
//     2-way: 0 ^ 0 == 1 ^ 1.)
//   * the MFMA runs on the unscaled e4m3 values; scale[n] meets the fp32 sums in the
//     epilogue, one rounding (K9q's rounding points).  EPI_PARTIAL (S > 1): fp32 slice z of
//     [S, M, N], already multiplied by scale[n], so splitk_reduce / splitk_reduce_silu /
//     splitk_add_rms_norm sum the slices unchanged (write-through stores, as K9m's); n is
//     the slice's column, so the slices of a SiLU-packed weight (columns in tile row order)
//     are given the scales in that order (ops/gemm.py _w8_packed_put).
//     EPI_OUT (S = 1): acc * scale[n] (+ bias[n]).  EPI_SILU (S = 1) over the SiLU-packed
//     merged [gate; up] weight (16-row groups of gate and up interleaved per tile):
//     silu(g * scale[row]) * (u * scale[I + row]) -> C [M, I].
// Rows >= M are never stored; their activation rows re-read row M - 1.
#include "common.h"
#include "launch.h"
#include <cstdlib>

namespace kgc {

namespace {

constexpr int QG_THREADS = 512;     // 8 waves: 4 along M x 2 along N
constexpr int QG_BK = 64, QG_BN = 128;
constexpr int QG_AROWB = 128;       // activation LDS row: 64 bf16 / f16
constexpr int QG_BROWB = 64;        // weight LDS row: 64 e4m3

enum { EPI_PARTIAL = 0, EPI_OUT = 1, EPI_SILU = 2 };

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
  if (younger >= D) { wait_vm<D * L>(); return; }
  if constexpr (D > 3) if (younger == 3) { wait_vm<3 * L>(); return; }
  if constexpr (D > 2) if (younger == 2) { wait_vm<2 * L>(); return; }
  if constexpr (D > 1) if (younger == 1) { wait_vm<L>(); return; }
  wait_vm<0>();
}

__device__ __forceinline__ float silu_f(float g) { return g / (1.f + __expf(-g)); }

// 16-B chunk position of (row, chunk) in a 128-B activation row (K9m's)
__device__ __host__ __forceinline__ int swz_a(int row, int chunk) { return chunk ^ (row & 7); }
// 16-B chunk position of (row, chunk) in a 64-B weight row: chunk ^ g((row / 4) % 4),
// g = (0, 2, 3, 1) packed two bits each into 0x78
__device__ __host__ __forceinline__ int swz_b(int row, int chunk) {
  return chunk ^ ((0x78 >> (((row >> 2) & 3) * 2)) & 3);
}

// weight row of tile row r (0..127) of column tile nb; SILU interleaves gate / up groups
template <bool SILU>
__device__ __forceinline__ int64_t weight_row(int nb, int r, int N) {
  if constexpr (SILU) {
    const int g = r >> 4;
    return (int64_t)((g & 1) ? (N >> 1) : 0) + nb * (QG_BN / 2) + (g >> 1) * 16 + (r & 15);
  } else {
    return (int64_t)nb * QG_BN + r;
  }
}

// write-through slice stores, as K9m's store_partial (KGC_PARTIAL_WT=0: plain stores)
__device__ __forceinline__ void store_partial(float* p, float v, int wt) {
  if (wt) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}

int partial_wt() {
  static const int v = [] {
    const char* e = getenv("KGC_PARTIAL_WT");
    return e ? atoi(e) : 1;
  }();
  return v;
}

template <typename T, int BM, int EPI, int NS>
__global__ __launch_bounds__(QG_THREADS, 1) void w8_dgemm_kernel(
    void* __restrict__ Cv, const T* __restrict__ X, const uint8_t* __restrict__ Wp,
    const float* __restrict__ scale, const T* __restrict__ bias, int M, int N, int K,
    int64_t ldx, int S, int MB, int64_t slice_stride, int wt) {
  constexpr int BN = QG_BN;
  constexpr int MT = BM / 4 / 16;                 // 16-row MFMA tiles per wave
  constexpr int NT = BN / 2 / 16;                 // 16-col MFMA tiles per wave
  constexpr int LA = BM / 8 / 8;                  // 1-KiB activation pieces per wave per step
  constexpr int LB = 1;                           // BN / 16 = 8 weight pieces: one per wave
  constexpr int L = LA + LB;
  constexpr int A_BYTES = BM * QG_AROWB, SLOT_BYTES = A_BYTES + BN * QG_BROWB;
  static_assert(BM % 64 == 0 && NT % 2 == 0, "wave tiling");
  static_assert(NS >= 3 && NS <= 6 && NS * SLOT_BYTES <= 163840, "LDS ring: 3..6 slots, 160 KiB");
  // one shared array for the whole ring (gemm_decode.hip)
  __shared__ __attribute__((aligned(16))) char lds[NS * SLOT_BYTES];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int z = blockIdx.x % S;
  const int j = blockIdx.x / S;
  const int mb = j % MB, nb = j / MB;
  const int m0 = mb * BM;

  // ---- DMA sources.  Activations: lane l of piece p fills LDS row 8p + l/8, position l%8
  // with global chunk (l%8) ^ (row%8); weights: the packed block, lane-linear
  const int drow = lane >> 3, dchunk = (lane & 7) ^ drow;
  const T* a_src[LA];
#pragma unroll
  for (int t = 0; t < LA; ++t) {
    int r = m0 + (wave * LA + t) * 8 + drow;
    r = r < M ? r : M - 1;                        // padded rows re-read the last row
    a_src[t] = X + (int64_t)r * ldx + dchunk * 8;
  }
  const int nk_all = K / QG_BK;
  const uint8_t* b_src = Wp + (int64_t)nb * nk_all * (BN * QG_BROWB) + wave * 1024 + lane * 16;

  const int kb0 = (int)((int64_t)nk_all * z / S);
  const int nk = (int)((int64_t)nk_all * (z + 1) / S) - kb0;
  // each workgroup starts its walk at its own step
  const int rot = nk >= 4 ? (int)(((int64_t)j * 37) % nk) : 0;

  auto issue = [&](int slot, int step) {
    char* sa = lds + slot * SLOT_BYTES;
    char* sb = sa + A_BYTES;
    int st = step + rot;
    st = st >= nk ? st - nk : st;
    const int kb = kb0 + st;
#pragma unroll
    for (int t = 0; t < LA; ++t) glds16<0>(a_src[t] + kb * QG_BK, sa + (wave * LA + t) * 1024);
    glds16<2>(b_src + (int64_t)kb * (BN * QG_BROWB), sb + wave * 1024);
  };

  f32x4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[i][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fq = lane >> 4;
  const int a_row0 = wm * (BM / 4) + fr;
  const int b_row0 = wn * (BN / 2) + fr;
  // the lane's channel scales (and bias), loaded before the K walk hides their latency
  // (the bias stays in its 16-bit form until the epilogue: widening it here would wait for it)
  float sc[NT];
  T bv[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int64_t wr = weight_row<EPI == EPI_SILU>(nb, b_row0 + n * 16, N);
    sc[n] = scale[wr];
    bv[n] = from_f<T>(0.f);
    if constexpr (EPI == EPI_OUT) {
      if (bias != nullptr) bv[n] = bias[wr];
    }
  }

  // NS-slot ring: NS - 1 steps issued ahead, NS - 2 of them in flight behind the one read
#pragma unroll
  for (int p = 0; p < NS - 1; ++p)
    if (p < nk) issue(p, p);
  int slot = 0;
  for (int it = 0; it < nk; ++it) {
    // step `it` must have landed; the (up to NS - 2) younger steps may stay in flight
    wait_younger<L, NS - 2>(nk - 1 - it);
    __builtin_amdgcn_s_barrier();
    // the slot read in iteration it - 1 (every wave has passed the barrier since)
    if (it + NS - 1 < nk) issue(slot == 0 ? NS - 1 : slot - 1, it + NS - 1);
    const char* sa = lds + slot * SLOT_BYTES;
    const char* sb = sa + A_BYTES;
    slot = slot == NS - 1 ? 0 : slot + 1;
    // 16 e4m3 per weight row and lane: k 8 fq + [0, 8) and 32 + 8 fq + [0, 8)
    Pack8<T> bfr[NT][2];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int r = b_row0 + n * 16;
      const u32x4 raw = *reinterpret_cast<const u32x4*>(sb + r * QG_BROWB + (swz_b(r, fq) << 4));
      bfr[n][0].u = fp8x8_widen<T>(u32x2{raw.x, raw.y});
      bfr[n][1].u = fp8x8_widen<T>(u32x2{raw.z, raw.w});
    }
#pragma unroll
    for (int ks = 0; ks < QG_BK / 32; ++ks) {
      const int c = ks * 4 + fq;
      Pack8<T> af[MT];
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const int r = a_row0 + i * 16;
        af[i].u = *reinterpret_cast<const u32x4*>(sa + r * QG_AROWB + (swz_a(r, c) << 4));
      }
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[i][n] = mfma16x16x32(af[i].v, bfr[n][ks].v, acc[i][n]);
    }
  }

  // ---- epilogue: lane holds C[4*fq + e][fr] of every 16x16 tile.  One wait for the
  // scales here, unconditionally (inside the per-row branches each row's wait would also
  // drain the previous rows' stores)
#pragma unroll
  for (int n = 0; n < NT; ++n) asm volatile("" : "+v"(sc[n]));
#pragma unroll
  for (int i = 0; i < MT; ++i) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int row = m0 + wm * (BM / 4) + i * 16 + fq * 4 + e;
      if (row >= M) continue;
      if constexpr (EPI == EPI_PARTIAL) {
        float* cp = reinterpret_cast<float*>(Cv) + z * slice_stride + (int64_t)row * N +
                    nb * BN + wn * (BN / 2) + fr;
#pragma unroll
        for (int n = 0; n < NT; ++n) store_partial(cp + n * 16, acc[i][n][e] * sc[n], wt);
      } else if constexpr (EPI == EPI_OUT) {
        T* cp = reinterpret_cast<T*>(Cv) + (int64_t)row * N + nb * BN + wn * (BN / 2) + fr;
#pragma unroll
        for (int n = 0; n < NT; ++n) cp[n * 16] = from_f<T>(acc[i][n][e] * sc[n] + to_f<T>(bv[n]));
      } else {
        const int I = N >> 1;
        T* cp = reinterpret_cast<T*>(Cv) + (int64_t)row * I + nb * (BN / 2) + wn * (BN / 4) + fr;
#pragma unroll
        for (int n = 0; n < NT; n += 2)
          cp[(n >> 1) * 16] =
              from_f<T>(silu_f(acc[i][n][e] * sc[n]) * (acc[i][n + 1][e] * sc[n + 1]));
      }
    }
  }
}

// Re-layout W8 [N, K] (silu: merged [gate; up]) into the packed tiles: 16-B chunk at
// position pos of tile row r of P[nb][kb] = W8[weight_row(nb, r)][kb*64 + 8q + [0, 8)]
// followed by [kb*64 + 32 + 8q + [0, 8)], q = swz_b(r, pos)  (ops/quant.py
// pack_fp8_tiles_reference is the same map in plain torch)
template <bool SILU>
__global__ __launch_bounds__(256) void w8_dgemm_pack_kernel(uint8_t* __restrict__ P,
                                                            const uint8_t* __restrict__ W, int N,
                                                            int K) {
  const int nk_all = K / QG_BK;
  const int64_t chunk = (int64_t)blockIdx.x * 256 + threadIdx.x;   // one 16-B chunk
  const int64_t total = (int64_t)N * K / 16;
  if (chunk >= total) return;
  const int pos = (int)(chunk & 3);
  const int64_t rowi = chunk >> 2;                 // (nb, kb, r) flattened
  const int r = (int)(rowi % QG_BN);
  const int64_t t = rowi / QG_BN;
  const int kb = (int)(t % nk_all);
  const int nb = (int)(t / nk_all);
  const int q = swz_b(r, pos);
  const uint8_t* src = W + weight_row<SILU>(nb, r, N) * K + kb * QG_BK + q * 8;
  const u32x2 lo = *reinterpret_cast<const u32x2*>(src);
  const u32x2 hi = *reinterpret_cast<const u32x2*>(src + 32);
  reinterpret_cast<u32x4*>(P)[chunk] = u32x4{lo.x, lo.y, hi.x, hi.y};
}

// Tile table: id -> (BM, ring slots); BN = 128 throughout.  Resource report (hipcc
// -Rpass-analysis=kernel-resource-usage, gfx950; bf16 and f16 alike, AGPRs 0, scratch 0
// everywhere), VGPRs for the slices / out / SiLU epilogue and waves per SIMD:
//   256 x 128, 3 slots (120 KB)   131 / 133 / 131   2
//   256 x 128, 4 slots (160 KB)   131 / 133 / 131   2
//   128 x 128, 3 slots ( 72 KB)    94 /  96 /  94   4
//   128 x 128, 4 slots ( 96 KB)    94 /  96 /  94   2
//   128 x 128, 6 slots (144 KB)    94 /  96 /  94   2
struct QgCfg {
  int bm, ns;
};
constexpr int kNumCfgs = 5;
static const QgCfg kCfg[kNumCfgs] = {{256, 3}, {256, 4}, {128, 3}, {128, 4}, {128, 6}};

template <typename T, int BM, int NS>
void w8_dgemm_cfg(int epi, void* C, const void* X, const void* Wp, const float* scale,
                  const void* bias, int M, int N, int K, int64_t ldx, int S, int64_t ss,
                  hipStream_t s) {
  const int MB = (M + BM - 1) / BM;
  const dim3 grid((unsigned)(MB * (N / QG_BN) * S));
#define QG_LAUNCH(EP)                                                                    \
  w8_dgemm_kernel<T, BM, EP, NS><<<grid, QG_THREADS, 0, s>>>(                            \
      C, (const T*)X, (const uint8_t*)Wp, scale, (const T*)bias, M, N, K, ldx, S, MB, ss, \
      partial_wt())
  if (epi == EPI_PARTIAL) QG_LAUNCH(EPI_PARTIAL);
  else if (epi == EPI_OUT) QG_LAUNCH(EPI_OUT);
  else QG_LAUNCH(EPI_SILU);
#undef QG_LAUNCH
}

template <typename T>
void w8_dgemm_t(int cfg, int epi, void* C, const void* X, const void* Wp, const float* scale,
                const void* bias, int M, int N, int K, int64_t ldx, int S, int64_t ss,
                hipStream_t s) {
  switch (cfg) {
    case 0: w8_dgemm_cfg<T, 256, 3>(epi, C, X, Wp, scale, bias, M, N, K, ldx, S, ss, s); break;
    case 1: w8_dgemm_cfg<T, 256, 4>(epi, C, X, Wp, scale, bias, M, N, K, ldx, S, ss, s); break;
    case 2: w8_dgemm_cfg<T, 128, 3>(epi, C, X, Wp, scale, bias, M, N, K, ldx, S, ss, s); break;
    case 3: w8_dgemm_cfg<T, 128, 4>(epi, C, X, Wp, scale, bias, M, N, K, ldx, S, ss, s); break;
    case 4: w8_dgemm_cfg<T, 128, 6>(epi, C, X, Wp, scale, bias, M, N, K, ldx, S, ss, s); break;
    default: break;                 // the host checks cfg < w8_dgemm_num_cfgs()
  }
}

}  // namespace

int w8_dgemm_num_cfgs() { return kNumCfgs; }
void w8_dgemm_cfg_info(int cfg, int* bm, int* bn, int* ns) {
  *bm = kCfg[cfg].bm;
  *bn = QG_BN;
  *ns = kCfg[cfg].ns;
}

void launch_w8_dgemm(int dtype, int cfg, int epi, void* C, const void* X, const void* Wp,
                     const float* scale, const void* bias, int M, int N, int K, int64_t ldx,
                     int S, int64_t slice_stride, hipStream_t s) {
  if (dtype == DT_BF16)
    w8_dgemm_t<bf16>(cfg, epi, C, X, Wp, scale, bias, M, N, K, ldx, S, slice_stride, s);
  else
    w8_dgemm_t<f16>(cfg, epi, C, X, Wp, scale, bias, M, N, K, ldx, S, slice_stride, s);
}

void launch_w8_dgemm_pack(bool silu, void* P, const void* W8, int N, int K, hipStream_t s) {
  const int64_t chunks = (int64_t)N * K / 16;
  if (chunks == 0) return;
  const dim3 grid((unsigned)((chunks + 255) / 256));
  if (silu)
    w8_dgemm_pack_kernel<true><<<grid, 256, 0, s>>>((uint8_t*)P, (const uint8_t*)W8, N, K);
  else
    w8_dgemm_pack_kernel<false><<<grid, 256, 0, s>>>((uint8_t*)P, (const uint8_t*)W8, N, K);
}

}  // namespace kgc
