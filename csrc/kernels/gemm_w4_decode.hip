// K9mf: the K9m mid-batch decode pipeline (gemm_decode.hip) over weight-only MXFP4 (W4A16)
// weights, for the decode buckets with 64 < M <= 512 of a --quantization mxfp4 model:
//
//   C[M, N] = X[M, K] . dq(W4)[N, K]^T               X / C bf16 or f16, W4 OCP MXFP4: e2m1
//                                                    codes, one e8m0 scale per 32 k of a row
//
// The structure is K9mq's (gemm_w8_decode.hip): 512-thread workgroups (4 (M) x 2 (N) waves
// of v_mfma_f32_16x16x32), BK = 64, BN = 128, both operands HBM/L2 -> LDS by LDS-DMA into a
// ring retired by counted `s_waitcnt vmcnt(N)` + a raw s_barrier, the weight stream
// non-temporal (aux = 2), each workgroup's K walk rotated, split-K over a 1-D grid with
// z = L % S, write-through slice stores.  The activation operand is K9mq's to the byte
// (128-B LDS rows, 16-B chunk c of row r at position c ^ (r % 8), the XOR on the DMA source
// address and on the read), so the A fragments are read exactly as K9m / K9mq read them.
// What differs is the weight operand, which stays 4-bit in LDS:
//   * a 64-k step of a weight row is 32 code bytes + 2 scale bytes, so a 128-row tile is
//     4096 + 256 = 4352 B and a 256 x 128 slot 32 + 4.25 = 36.25 KB (128 x 128: 20.25 KB);
//   * PACKED weights only (w4_dgemm_pack): tiles [N/128][K/64][4352 B], one contiguous block
//     per K-step of a column tile, copied lane-linear: the 4096 code bytes by four 1-KiB
//     16-byte DMAs (waves 0-3, one each), the 256 scale bytes by ONE 4-byte-wide DMA
//     (wave 4: 64 lanes x 4 B, full EXEC).  No byte- or short-sized load and no ordinary
//     global load inside the K loop;
//   * codes: 32-B rows of four 8-byte chunks.  Chunk q of a row is the dword of codes at
//     k = 8q + [0, 8) (the lane's B fragment of MFMA ks = 0) followed by the dword at
//     k = 32 + 8q + [0, 8) (ks = 1): lane (r16, q4) reads ONE ds_read_b64 per row and step.
//     Chunk q of tile row r sits at position q ^ (2 * ((r >> 3) & 1)), baked into the packed
//     tiles and applied on the read.  Bank argument (bank (a / 4) % 64, a ds_read_b64 is
//     served in two 32-lane halves): the 256-B bank row holds 8 code rows, so the 8-byte slot
//     of (r, position p) is 4 (r % 8) + p, and tile rows r and r + 8 share their slots.  Half
//     0 is lanes q4 = 0, 1 of the wave's 16 rows: rows 0-7 read positions {0, 1}, rows 8-15
//     positions {0, 1} ^ 2 = {2, 3} -- 32 lanes on 32 distinct slots.  Half 1 (q4 = 2, 3) is
//     the same with the position sets swapped.  The n-tile and wave offsets are multiples of
//     16 rows = 512 B and change neither the bank nor (r >> 3) & 1.  (Unswizzled, rows r and
//     r + 8 of a half share a slot: 2-way.);
//   * scales: the step's 256 e8m0 bytes as [wn][r16][n-tile][ks], so lane (r16, q4) of
//     N-wave wn reads the scales of its four rows and both MFMA halves with ONE ds_read_b64
//     at 128 wn + 8 r16.  Bank argument: the four q4 lanes of a row read one address
//     (broadcast), and the 16 addresses of a half are 16 distinct 8-byte slots of one 128-B
//     span: conflict-free;
//   * each code dword is widened by fp4x8_widen (v_cvt_scalef32_pk_{bf16,f16}_fp4) with the
//     fp32 scale 2^(b - 127) of ITS block (MFMA half ks of the step is scale block ks): the
//     conversion multiplies by a power of two, so the MFMA operand is the exact dequantised
//     value, the epilogue carries no scale and the only rounding is the output's;
//   * the waves issue different numbers of DMAs per step (activation pieces + one for waves
//     0-4, + none for waves 5-7), so the counted wait is per wave: wave w waits until at
//     most min(NS - 2, younger steps) x L_w of ITS OWN DMAs are in flight, L_w its DMAs per
//     step.  vmcnt retires in issue order within a wave, so that wait retires exactly the
//     wave's DMAs of the step about to be read and none younger; the s_barrier that follows
//     makes it hold for every wave's part of that step.
// Epilogues: EPI_PARTIAL (S > 1) fp32 slice z of [S, M, N] (write-through stores, summed by
// splitk_reduce / splitk_reduce_silu / splitk_add_rms_norm); EPI_OUT (S = 1) acc (+ bias[n]),
// rounded once; EPI_SILU (S = 1) over the SiLU-packed merged [gate; up] weight (16-row
// groups of gate and up interleaved per tile): silu(g) * u -> C [M, N/2].  The slices of a
// SiLU-packed weight come out in tile row order (splitk_reduce_silu(interleaved = true)).
// Rows >= M are never stored; their activation rows re-read row M - 1.
#include "common.h"
#include "launch.h"
#include <cstdlib>

namespace kgc {

namespace {

constexpr int FG_THREADS = 512;     // 8 waves: 4 along M x 2 along N
constexpr int FG_BK = 64, FG_BN = 128;
constexpr int FG_AROWB = 128;       // activation LDS row: 64 bf16 / f16
constexpr int FG_BROWB = 32;        // weight LDS row: 64 e2m1
constexpr int FG_CODEB = FG_BN * FG_BROWB;          // 4096 code bytes per tile
constexpr int FG_TILEB = FG_CODEB + 2 * FG_BN;      // + 256 scale bytes

enum { EPI_PARTIAL = 0, EPI_OUT = 1, EPI_SILU = 2 };

typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void gbl_void;

template <int AUX>
__device__ __forceinline__ void glds16(const void* src, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((gbl_void*)src, (lds_void*)lds_wave_base, 16, 0, AUX);
}
template <int AUX>
__device__ __forceinline__ void glds4(const void* src, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((gbl_void*)src, (lds_void*)lds_wave_base, 4, 0, AUX);
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
// 8-B chunk position of (row, chunk) in a 32-B code row
__device__ __host__ __forceinline__ int swz_b(int row, int chunk) {
  return chunk ^ (((row >> 3) & 1) << 1);
}

// weight row of tile row r (0..127) of column tile nb; SILU interleaves gate / up groups
template <bool SILU>
__device__ __forceinline__ int64_t weight_row(int nb, int r, int N) {
  if constexpr (SILU) {
    const int g = r >> 4;
    return (int64_t)((g & 1) ? (N >> 1) : 0) + nb * (FG_BN / 2) + (g >> 1) * 16 + (r & 15);
  } else {
    return (int64_t)nb * FG_BN + r;
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
__global__ __launch_bounds__(FG_THREADS, 1) void w4_dgemm_kernel(
    void* __restrict__ Cv, const T* __restrict__ X, const uint8_t* __restrict__ Wp,
    const T* __restrict__ bias, int M, int N, int K, int64_t ldx, int S, int MB,
    int64_t slice_stride, int wt) {
  constexpr int BN = FG_BN;
  constexpr int MT = BM / 4 / 16;                 // 16-row MFMA tiles per wave
  constexpr int NT = BN / 2 / 16;                 // 16-col MFMA tiles per wave
  constexpr int LA = BM / 8 / 8;                  // 1-KiB activation pieces per wave per step
  constexpr int A_BYTES = BM * FG_AROWB, SLOT_BYTES = A_BYTES + FG_TILEB;
  static_assert(BM % 64 == 0 && NT == 4, "wave tiling (the scale block holds 4 n-tiles)");
  static_assert(NS >= 3 && NS <= 6 && NS * SLOT_BYTES <= 163840, "LDS ring: 3..6 slots, 160 KiB");
  // one shared array for the whole ring (gemm_decode.hip)
  __shared__ __attribute__((aligned(16))) char lds[NS * SLOT_BYTES];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: the branches on it
  const int wm = wave >> 1, wn = wave & 1;
  const int z = blockIdx.x % S;
  const int j = blockIdx.x / S;
  const int mb = j % MB, nb = j / MB;
  const int m0 = mb * BM;

  // ---- DMA sources.  Activations: lane l of piece p fills LDS row 8p + l/8, position l%8
  // with global chunk (l%8) ^ (row%8); weights: the packed block, lane-linear -- waves 0-3
  // a 1-KiB piece of the codes each, wave 4 the 256 scale bytes, waves 5-7 nothing
  const int drow = lane >> 3, dchunk = (lane & 7) ^ drow;
  const T* a_src[LA];
#pragma unroll
  for (int t = 0; t < LA; ++t) {
    int r = m0 + (wave * LA + t) * 8 + drow;
    r = r < M ? r : M - 1;                        // padded rows re-read the last row
    a_src[t] = X + (int64_t)r * ldx + dchunk * 8;
  }
  const int nk_all = K / FG_BK;
  const uint8_t* b_src = Wp + (int64_t)nb * nk_all * FG_TILEB +
                         (wave < 4 ? wave * 1024 + lane * 16 : FG_CODEB + lane * 4);

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
    for (int t = 0; t < LA; ++t) glds16<0>(a_src[t] + kb * FG_BK, sa + (wave * LA + t) * 1024);
    if (wave < 4) glds16<2>(b_src + (int64_t)kb * FG_TILEB, sb + wave * 1024);
    else if (wave == 4) glds4<2>(b_src + (int64_t)kb * FG_TILEB, sb + FG_CODEB);
  };

  f32x4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[i][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fq = lane >> 4;
  const int a_row0 = wm * (BM / 4) + fr;
  const int b_row0 = wn * (BN / 2) + fr;
  // the lane's code chunk of each n-tile, as an offset in the slot.  The offsets pass through
  // an empty asm so that the compiler sees four unrelated addresses: it would otherwise fuse
  // the reads pairwise into ds_read2st64_b64, which runs at half ds_read_b64's rate and
  // banks modulo 32 (where rows r and r + 4 collide)
  int b_off[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int r = b_row0 + n * 16;
    b_off[n] = A_BYTES + r * FG_BROWB + (swz_b(r, fq) << 3);
    asm volatile("" : "+v"(b_off[n]));
  }
  // the lane's bias, loaded before the K walk hides its latency (it stays in its 16-bit
  // form until the epilogue: widening it here would wait for it)
  T bv[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    bv[n] = from_f<T>(0.f);
    if constexpr (EPI == EPI_OUT) {
      if (bias != nullptr) bv[n] = bias[weight_row<false>(nb, b_row0 + n * 16, N)];
    }
  }

  // NS-slot ring: NS - 1 steps issued ahead, NS - 2 of them in flight behind the one read
#pragma unroll
  for (int p = 0; p < NS - 1; ++p)
    if (p < nk) issue(p, p);
  int slot = 0;
  for (int it = 0; it < nk; ++it) {
    // step `it` must have landed; the (up to NS - 2) younger steps may stay in flight.  The
    // count is the wave's own DMAs per step (header): the wait retires exactly this wave's
    // part of step `it`, the barrier every other wave's
    if (wave < 5) wait_younger<LA + 1, NS - 2>(nk - 1 - it);
    else wait_younger<LA, NS - 2>(nk - 1 - it);
    __builtin_amdgcn_s_barrier();
    // the slot read in iteration it - 1 (every wave has passed the barrier since)
    if (it + NS - 1 < nk) issue(slot == 0 ? NS - 1 : slot - 1, it + NS - 1);
    const char* sa = lds + slot * SLOT_BYTES;
    const char* sb = sa + A_BYTES;
    slot = slot == NS - 1 ? 0 : slot + 1;
    // per weight row and lane: the code dwords of k 8 fq + [0, 8) and 32 + 8 fq + [0, 8),
    // widened with the scales of blocks 0 and 1 of the step
    const u32x2 sd = *reinterpret_cast<const u32x2*>(sb + FG_CODEB + wn * 128 + fr * 8);
    Pack8<T> bfr[NT][2];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const u32x2 raw = *reinterpret_cast<const u32x2*>(sa + b_off[n]);
      const uint32_t sw = (n & 2) ? sd.y : sd.x;
      bfr[n][0].u = fp4x8_widen<T>(raw.x, e8m0_f32(sw, (n & 1) * 2));
      bfr[n][1].u = fp4x8_widen<T>(raw.y, e8m0_f32(sw, (n & 1) * 2 + 1));
    }
#pragma unroll
    for (int ks = 0; ks < FG_BK / 32; ++ks) {
      const int c = ks * 4 + fq;
      Pack8<T> af[MT];
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const int r = a_row0 + i * 16;
        af[i].u = *reinterpret_cast<const u32x4*>(sa + r * FG_AROWB + (swz_a(r, c) << 4));
      }
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[i][n] = mfma16x16x32(af[i].v, bfr[n][ks].v, acc[i][n]);
    }
  }

  // ---- epilogue: lane holds C[4*fq + e][fr] of every 16x16 tile.  One wait for the bias
  // here, unconditionally (inside the per-row branches each row's wait would also drain the
  // previous rows' stores)
  if constexpr (EPI == EPI_OUT) {
#pragma unroll
    for (int n = 0; n < NT; ++n) asm volatile("" : "+v"(bv[n]));
  }
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
        for (int n = 0; n < NT; ++n) store_partial(cp + n * 16, acc[i][n][e], wt);
      } else if constexpr (EPI == EPI_OUT) {
        T* cp = reinterpret_cast<T*>(Cv) + (int64_t)row * N + nb * BN + wn * (BN / 2) + fr;
#pragma unroll
        for (int n = 0; n < NT; ++n) cp[n * 16] = from_f<T>(acc[i][n][e] + to_f<T>(bv[n]));
      } else {
        const int I = N >> 1;
        T* cp = reinterpret_cast<T*>(Cv) + (int64_t)row * I + nb * (BN / 2) + wn * (BN / 4) + fr;
#pragma unroll
        for (int n = 0; n < NT; n += 2)
          cp[(n >> 1) * 16] = from_f<T>(silu_f(acc[i][n][e]) * acc[i][n + 1][e]);
      }
    }
  }
}

// Re-layout the OCP codes W4 [N, K/2] and scales Sc [N, K/32] (silu: merged [gate; up]) into
// the packed tiles, one pass: tile P[nb][kb] is 512 8-byte code chunks -- the chunk at
// position pos of tile row r = the 4 code bytes of k = kb*64 + 8q + [0, 8) of weight row
// weight_row(nb, r) followed by those of k = kb*64 + 32 + 8q + [0, 8), q = swz_b(r, pos) --
// then 64 scale dwords: dword (wn, r16, h) = the scale bytes (n-tile 2h, ks 0), (2h, 1),
// (2h + 1, 0), (2h + 1, 1) of tile row 64 wn + 16 n + r16, ks the 32-k block of the step
// (ops/quant.py pack_mxfp4_tiles_reference is the same map in plain torch)
template <bool SILU>
__global__ __launch_bounds__(256) void w4_dgemm_pack_kernel(uint8_t* __restrict__ P,
                                                            const uint8_t* __restrict__ W,
                                                            const uint8_t* __restrict__ Sc,
                                                            int N, int K) {
  constexpr int UNITS = FG_CODEB / 8 + FG_BN / 2;  // 512 code chunks + 64 scale dwords
  const int nk_all = K / FG_BK;
  const int64_t unit = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t total = (int64_t)(N / FG_BN) * nk_all * UNITS;
  if (unit >= total) return;
  const int u = (int)(unit % UNITS);
  const int64_t t = unit / UNITS;                  // (nb, kb) flattened
  const int kb = (int)(t % nk_all);
  const int nb = (int)(t / nk_all);
  uint8_t* tile = P + t * FG_TILEB;
  if (u < FG_CODEB / 8) {
    const int r = u >> 2, q = swz_b(r, u & 3);
    const uint8_t* src = W + weight_row<SILU>(nb, r, N) * (K / 2) + kb * (FG_BK / 2) + q * 4;
    const uint32_t lo = *reinterpret_cast<const uint32_t*>(src);
    const uint32_t hi = *reinterpret_cast<const uint32_t*>(src + 16);
    *reinterpret_cast<u32x2*>(tile + u * 8) = u32x2{lo, hi};
  } else {
    const int s = u - FG_CODEB / 8;
    const int wn = s >> 5, r16 = (s >> 1) & 15, h = s & 1;
    uint32_t dw = 0;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int r = wn * (FG_BN / 2) + (2 * h + b) * 16 + r16;
      const uint8_t* src = Sc + weight_row<SILU>(nb, r, N) * (K / 32) + kb * 2;
      dw |= (uint32_t)*reinterpret_cast<const uint16_t*>(src) << (16 * b);
    }
    *reinterpret_cast<uint32_t*>(tile + FG_CODEB + s * 4) = dw;
  }
}

// Tile table: id -> (BM, ring slots); BN = 128 throughout.  Resource report (hipcc
// -Rpass-analysis=kernel-resource-usage, gfx950; bf16 and f16 alike, AGPRs 0, scratch 0
// everywhere), VGPRs for the slices / out / SiLU epilogue and waves per SIMD:
//   256 x 128, 3 slots (108.75 KB)   120 / 122 / 120   2
//   256 x 128, 4 slots (145 KB)      120 / 122 / 120   2
//   128 x 128, 3 slots ( 60.75 KB)    84 /  86 /  84   4
//   128 x 128, 4 slots ( 81 KB)       84 /  86 /  84   2
//   128 x 128, 6 slots (121.5 KB)     84 /  86 /  84   2
// Inner loop of 256 x 128 (per wave and step): 32 MFMA, 32 v_cvt_scalef32_pk_*_fp4, 8
// ds_read_b128 (activations) + 5 ds_read_b64 (4 code chunks, 1 scale block), 4 or 5 LDS-DMAs,
// no other load; w4_dgemm_pack 13 VGPRs, 8 waves per SIMD.
struct FgCfg {
  int bm, ns;
};
constexpr int kNumCfgs = 5;
static const FgCfg kCfg[kNumCfgs] = {{256, 3}, {256, 4}, {128, 3}, {128, 4}, {128, 6}};

template <typename T, int BM, int NS>
void w4_dgemm_cfg(int epi, void* C, const void* X, const void* Wp, const void* bias, int M,
                  int N, int K, int64_t ldx, int S, int64_t ss, hipStream_t s) {
  const int MB = (M + BM - 1) / BM;
  const dim3 grid((unsigned)(MB * (N / FG_BN) * S));
#define FG_LAUNCH(EP)                                                                 \
  w4_dgemm_kernel<T, BM, EP, NS><<<grid, FG_THREADS, 0, s>>>(                         \
      C, (const T*)X, (const uint8_t*)Wp, (const T*)bias, M, N, K, ldx, S, MB, ss,    \
      partial_wt())
  if (epi == EPI_PARTIAL) FG_LAUNCH(EPI_PARTIAL);
  else if (epi == EPI_OUT) FG_LAUNCH(EPI_OUT);
  else FG_LAUNCH(EPI_SILU);
#undef FG_LAUNCH
}

template <typename T>
void w4_dgemm_t(int cfg, int epi, void* C, const void* X, const void* Wp, const void* bias,
                int M, int N, int K, int64_t ldx, int S, int64_t ss, hipStream_t s) {
  switch (cfg) {
    case 0: w4_dgemm_cfg<T, 256, 3>(epi, C, X, Wp, bias, M, N, K, ldx, S, ss, s); break;
    case 1: w4_dgemm_cfg<T, 256, 4>(epi, C, X, Wp, bias, M, N, K, ldx, S, ss, s); break;
    case 2: w4_dgemm_cfg<T, 128, 3>(epi, C, X, Wp, bias, M, N, K, ldx, S, ss, s); break;
    case 3: w4_dgemm_cfg<T, 128, 4>(epi, C, X, Wp, bias, M, N, K, ldx, S, ss, s); break;
    case 4: w4_dgemm_cfg<T, 128, 6>(epi, C, X, Wp, bias, M, N, K, ldx, S, ss, s); break;
    default: break;                 // the host checks cfg < w4_dgemm_num_cfgs()
  }
}

}  // namespace

int w4_dgemm_num_cfgs() { return kNumCfgs; }
void w4_dgemm_cfg_info(int cfg, int* bm, int* bn, int* ns) {
  *bm = kCfg[cfg].bm;
  *bn = FG_BN;
  *ns = kCfg[cfg].ns;
}

void launch_w4_dgemm(int dtype, int cfg, int epi, void* C, const void* X, const void* Wp,
                     const void* bias, int M, int N, int K, int64_t ldx, int S,
                     int64_t slice_stride, hipStream_t s) {
  if (dtype == DT_BF16)
    w4_dgemm_t<bf16>(cfg, epi, C, X, Wp, bias, M, N, K, ldx, S, slice_stride, s);
  else
    w4_dgemm_t<f16>(cfg, epi, C, X, Wp, bias, M, N, K, ldx, S, slice_stride, s);
}

void launch_w4_dgemm_pack(bool silu, void* P, const void* W4, const void* scales, int N, int K,
                          hipStream_t s) {
  const int64_t units = (int64_t)(N / FG_BN) * (K / FG_BK) * (FG_CODEB / 8 + FG_BN / 2);
  if (units == 0) return;
  const dim3 grid((unsigned)((units + 255) / 256));
  if (silu)
    w4_dgemm_pack_kernel<true><<<grid, 256, 0, s>>>((uint8_t*)P, (const uint8_t*)W4,
                                                    (const uint8_t*)scales, N, K);
  else
    w4_dgemm_pack_kernel<false><<<grid, 256, 0, s>>>((uint8_t*)P, (const uint8_t*)W4,
                                                     (const uint8_t*)scales, N, K);
}

}  // namespace kgc
