// K9f: weight-only MXFP4 (W4A16) skinny GEMM for small-batch decode on gfx950:
//   C[M, N] = X[M, K] . dq(W4)[N, K]^T (+ bias),  M <= 64,
// W4 the OCP MX v1.0 form of a linear layer's [out, in] weight (ops/quant.py quantize_mxfp4):
// codes uint8 [N, K/2], element 2j the low and 2j+1 the high nibble of byte j (e2m1: sign bit
// 3, magnitude bits 2..0), and e8m0 block scales uint8 [N, K/32], one per 32 consecutive k of
// a row.  X / C / bias bf16 or f16.
//
// The structure is K9's (gemm_skinny.hip) by way of K9q (gemm_w8.hip): a workgroup owns
// 16*NT weight rows and ALL of K, its NW waves split K evenly, two register sets of loads are
// in flight, the weights stream as non-temporal 16-byte loads, the per-wave partial sums merge
// in LDS and the workgroup writes coalesced rows of C.  What differs:
//   * a 16-byte load is 32 e2m1 -- exactly one scale block of one row -- and becomes the A
//     fragments of FOUR v_mfma_f32_16x16x32 (a "unit", 128 k per wave): dword j of the load
//     widens (v_cvt_scalef32_pk_{bf16,f16}_fp4, one byte -> one packed pair, the fp32 scale
//     2^(b-127) = b << 23 applied by the conversion) into the 8 k of MFMA j.  The conversion
//     multiplies by a power of two, so the MFMA operand is the exact dequantised value: no
//     scale in the epilogue, the only rounding is the output's;
//   * lane (r16, q4) walks 128 consecutive k of its row per 512-k "step" of the wave: four
//     16-byte weight loads and ONE 4-byte load of their four scale bytes.  A register set
//     holds U of the step's four units (U = 4 / 2 / 1 at MT = 1 / 2 / 4: the X fragments of
//     a unit are 16 VGPRs per batch tile); each set loads the step's scale dword itself (the
//     same 4 bytes 4 / U times: one more load instruction, no more HBM traffic, and no
//     byte-sized load in the loop).  The X fragments (B operand) use the same k-permutation;
//   * a wave's K-range that is no multiple of 512 ends in up to three single units with the
//     k of lane q4 at 32 q4 and a one-byte scale load each (outside the main loop);
//   * two epilogues: plain (+ bias), and W4_SILU over a merged [gate; up] weight [2I, K]
//     (n-tile 0 streams gate rows g0.., n-tile 1 the up rows I+g0..): C[m, g] = silu(gate) *
//     up, C [M, I].
// Shapes (checked on the host): N % (16*NT) == 0, K % (128*NW) == 0, 16-byte aligned rows.
//
// Configurations (mt, nt, nw) in {1,2,4} x {1,2} x {2,4,8} without (4,2,8), whose LDS partial
// sums would be 64 KB: it is not built and w4_ok rejects it.  Compiler resource report (hipcc
// -O3, gfx950; bf16 = f16; the SiLU forms within one VGPR of their plain forms), VGPR+AGPR,
// scratch 0 and 2 waves per SIMD for every one -- nothing spills:
//   (1,1,2) 194+4   (1,1,4) 194+4   (1,1,8) 200     (1,2,2) 238+8   (1,2,4) 238+8   (1,2,8) 248
//   (2,1,2) 182+8   (2,1,4) 182+8   (2,1,8) 192     (2,2,2) 222+16  (2,2,4) 222+16  (2,2,8) 240
//   (4,1,2) 178+16  (4,1,4) 178+16  (4,1,8) 194     (4,2,2) 208+32  (4,2,4) 208+32
//   w4_widen 23 VGPRs, 8 waves per SIMD.
// Inner loop of (1,1,4), two batches: 32 MFMA, 128 v_cvt_scalef32_pk_bf16_fp4 (4 per MFMA),
// 8 weight + 32 X 16-byte loads, 2 scale dwords, no byte-sized load, 17 counted s_waitcnt.
//
// Measured (profiles/w4_gemm_vs_fp8.jsonl): at M <= 16 K9f runs in K9q's time, within -8 .. +11 %,
// although it streams 0.53x the bytes: per weight ELEMENT it issues what K9q issues (one
// conversion per two elements, one MFMA and one 16-byte X load per eight), which points at
// that per-element work, not the weight stream, as what bounds both kernels at these shapes
// (a reading of the timings: no counter run was made).  Two variants were measured and
// dropped because they changed nothing: X through a range-checked buffer descriptor so that
// lanes of batch rows >= M load nothing, and register sets of half the depth (112 VGPRs,
// 4 waves per SIMD).
//
// w4_widen: out[n, k] = dq(W4)[n, k] in bf16 / f16, exact -- prefill, and the M > 64 that K9mf
// (gemm_w4_decode.hip) does not run, widen a weight into a static scratch and run the library
// GEMM on it.
#include "common.h"
#include "launch.h"

namespace kgc {

// (fp4x8_widen and e8m0_f32 live in common.h: K9mf, gemm_w4_decode.hip, widens the same way)

template <typename T, int MT, int NT, int NW, bool SILU>
__global__ __launch_bounds__(NW * 64) void w4_gemm_kernel(
    T* __restrict__ C, const T* __restrict__ X, const uint8_t* __restrict__ W,
    const uint8_t* __restrict__ S, const T* __restrict__ bias, int M, int K, int64_t ldx,
    int64_t ldc) {
  static_assert(!SILU || NT == 2, "W4_SILU pairs n-tile 0 (gate) with n-tile 1 (up)");
  constexpr int U = MT == 1 ? 4 : (MT == 2 ? 2 : 1);   // units per register set
  __shared__ __attribute__((aligned(16))) float red[NW][MT][NT][64][4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r16 = lane & 15, q4 = lane >> 4;
  // W4_SILU: gridDim.x = I / 16 workgroups over the I = 16 * gridDim.x output columns
  const int64_t n0 = (int64_t)blockIdx.x * (SILU ? 16 : 16 * NT);
  const int64_t n_half = SILU ? (int64_t)gridDim.x * 16 : 0;
  const int kw = K / NW;
  const int kbeg = wave * kw, kend = kbeg + kw;

  const uint8_t* wrow[NT];   // codes and scales of this lane's row, at k = 0
  const uint8_t* srow[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int64_t n = n0 + (SILU ? nt * n_half : 16 * nt) + r16;
    wrow[nt] = W + n * (int64_t)(K / 2);
    srow[nt] = S + n * (int64_t)(K / 32);
  }
  const T* xrow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) xrow[mt] = X + (int64_t)min(16 * mt + r16, M - 1) * ldx;

  f32x4 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // one unit: 32 e2m1 per weight row widened into four A fragments, four MFMAs per tile
  auto unit = [&](const u32x4* wf, const float* sc, const Pack8<T> (*xf)[4]) {
    Pack8<T> a[NT][4];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      a[nt][0].u = fp4x8_widen<T>(wf[nt].x, sc[nt]);
      a[nt][1].u = fp4x8_widen<T>(wf[nt].y, sc[nt]);
      a[nt][2].u = fp4x8_widen<T>(wf[nt].z, sc[nt]);
      a[nt][3].u = fp4x8_widen<T>(wf[nt].w, sc[nt]);
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[mt][nt] = mfma16x16x32(a[nt][j].v, xf[mt][j].v, acc[mt][nt]);
  };

  typedef u32x4 WSet[U][NT];
  typedef uint32_t SSet[NT];
  typedef Pack8<T> XSet[U][MT][4];
  // batch bi: units [U bi, U bi + U) of the wave's K-range; unit g is sub-block g % 4 of
  // step g / 4, where lane q4 holds k = kbeg + 512 (g / 4) + 128 q4 + 32 (g % 4) + [0, 32)
  auto load = [&](WSet& wf, SSet& sd, XSet& xf, int bi) {
    const int g0 = bi * U;
    const int ks = kbeg + 512 * (g0 >> 2);                 // the step's first k
    const int kl = ks + 128 * q4 + 32 * (g0 & 3);          // this lane's, unit 0 of the batch
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        wf[u][nt] = __builtin_nontemporal_load(
            reinterpret_cast<const u32x4*>(wrow[nt] + (kl >> 1) + 16 * u));
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      sd[nt] = *reinterpret_cast<const uint32_t*>(srow[nt] + (ks >> 5) + 4 * q4);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          xf[u][mt][j].u = *reinterpret_cast<const u32x4*>(xrow[mt] + kl + 32 * u + 8 * j);
  };
  auto compute = [&](const WSet& wf, const SSet& sd, const XSet& xf, int bi) {
    const int sub0 = (bi * U) & 3;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float sc[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) sc[nt] = e8m0_f32(sd[nt], sub0 + u);
      unit(wf[u], sc, xf[u]);
    }
  };
  // two register sets (A, B): batch b+1's loads are in flight while batch b's MFMAs wait
  // only for their own (the compiler's wait-count pass places the counted waits)
  const int nb = (kw / 512) * (4 / U);
  WSet wa, wb;
  SSet sa, sb;
  XSet xa, xb;
  if (nb > 0) load(wa, sa, xa, 0);
  for (int b = 0; b < nb; b += 2) {
    if (b + 1 < nb) load(wb, sb, xb, b + 1);
    compute(wa, sa, xa, b);
    if (b + 1 < nb) {
      if (b + 2 < nb) load(wa, sa, xa, b + 2);
      compute(wb, sb, xb, b + 1);
    }
  }
  // K-range not a multiple of 512: single units, lane q4 at k + 32 q4, one scale byte each
  for (int k = kbeg + (kw / 512) * 512; k < kend; k += 128) {
    const int kl = k + 32 * q4;
    u32x4 wf[NT];
    float sc[NT];
    Pack8<T> xf[MT][4];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      wf[nt] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wrow[nt] + (kl >> 1)));
      sc[nt] = e8m0_f32(srow[nt][kl >> 5], 0);
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        xf[mt][j].u = *reinterpret_cast<const u32x4*>(xrow[mt] + kl + 8 * j);
    unit(wf, sc, xf);
  }

  // ---- merge the NW K-slices: lane (r16, q4) of wave w holds C^T[16nt+4q4+i][16mt+r16]
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      *reinterpret_cast<f32x4*>(&red[wave][mt][nt][lane][0]) = acc[mt][nt];
  __syncthreads();
  constexpr int TN = SILU ? 16 : 16 * NT;
  const int rows = min(M, 16 * MT);
  for (int e = threadIdx.x; e < rows * TN; e += NW * 64) {
    const int m = e / TN, n = e % TN;
    const int mt = m >> 4, nt = n >> 4, nn = n & 15;
    const int l = (nn >> 2) * 16 + (m & 15), i = nn & 3;
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += red[w][mt][nt][l][i];
    if constexpr (SILU) {
      float u = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) u += red[w][mt][1][l][i];
      C[(int64_t)m * ldc + n0 + n] = from_f<T>(s / (1.f + __expf(-s)) * u);
    } else {
      if (bias != nullptr) s += to_f<T>(bias[n0 + n]);
      C[(int64_t)m * ldc + n0 + n] = from_f<T>(s);
    }
  }
}

template <typename T, int MT, int NT, int NW>
static void w4_go(bool silu, dim3 grid, hipStream_t s, void* C, const void* X, const void* W,
                  const void* S, const void* bias, int M, int K, int64_t ldx, int64_t ldc) {
#define W4_GO(SILU_)                                                                     \
  w4_gemm_kernel<T, MT, NT, NW, SILU_><<<grid, NW * 64, 0, s>>>(                         \
      (T*)C, (const T*)X, (const uint8_t*)W, (const uint8_t*)S, (const T*)bias, M, K, ldx, ldc)
  if constexpr (NT == 2) {
    if (silu) {
      W4_GO(true);
      return;
    }
  }
  W4_GO(false);
#undef W4_GO
}

template <typename T, int MT>
static void w4_mt(int nt, int nw, bool silu, void* C, const void* X, const void* W,
                  const void* S, const void* bias, int M, int N, int K, int64_t ldx,
                  int64_t ldc, hipStream_t s) {
  const dim3 grid(silu ? N / 32 : N / (16 * nt));   // silu: N = 2I
#define W4_NW(NT_, NW_) w4_go<T, MT, NT_, NW_>(silu, grid, s, C, X, W, S, bias, M, K, ldx, ldc)
  if (nt == 2) {
    // (mt, nt, nw) = (4, 2, 8) is not built (64 KB of LDS partials); the host rejects it
    if (nw == 8) {
      if constexpr (MT < 4) W4_NW(2, 8);
    } else if (nw == 4) W4_NW(2, 4);
    else W4_NW(2, 2);
  } else {
    if (nw == 8) W4_NW(1, 8);
    else if (nw == 4) W4_NW(1, 4);
    else W4_NW(1, 2);
  }
#undef W4_NW
}

template <typename T>
static void w4_t(int mt, int nt, int nw, bool silu, void* C, const void* X, const void* W,
                 const void* S, const void* bias, int M, int N, int K, int64_t ldx, int64_t ldc,
                 hipStream_t s) {
  if (mt == 1) w4_mt<T, 1>(nt, nw, silu, C, X, W, S, bias, M, N, K, ldx, ldc, s);
  else if (mt == 2) w4_mt<T, 2>(nt, nw, silu, C, X, W, S, bias, M, N, K, ldx, ldc, s);
  else w4_mt<T, 4>(nt, nw, silu, C, X, W, S, bias, M, N, K, ldx, ldc, s);
}

void launch_w4_gemm(int dtype, int mt, int nt, int nw, bool silu, void* C, const void* X,
                    const void* W, const void* S, const void* bias, int M, int N, int K,
                    int64_t ldx, int64_t ldc, hipStream_t s) {
  if (M == 0 || N == 0) return;
  if (dtype == DT_BF16) w4_t<bf16>(mt, nt, nw, silu, C, X, W, S, bias, M, N, K, ldx, ldc, s);
  else w4_t<f16>(mt, nt, nw, silu, C, X, W, S, bias, M, N, K, ldx, ldc, s);
}

// ---- w4_widen: one scale block per thread: 16 bytes of codes -> 32 T, exact.  Block c of
// the row-major codes is scale byte c of the row-major scales.
template <typename T>
__global__ __launch_bounds__(256) void w4_widen_kernel(T* __restrict__ out,
                                                       const uint8_t* __restrict__ W,
                                                       const uint8_t* __restrict__ S,
                                                       int64_t blocks) {
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < blocks;
       c += (int64_t)gridDim.x * 256) {
    const float sc = e8m0_f32(S[c], 0);
    const u32x4 raw = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(W + c * 16));
    u32x4* dst = reinterpret_cast<u32x4*>(out + c * 32);
    dst[0] = fp4x8_widen<T>(raw.x, sc);
    dst[1] = fp4x8_widen<T>(raw.y, sc);
    dst[2] = fp4x8_widen<T>(raw.z, sc);
    dst[3] = fp4x8_widen<T>(raw.w, sc);
  }
}

void launch_w4_widen(int dtype, void* out, const void* W, const void* S, int64_t N, int64_t K,
                     hipStream_t s) {
  const int64_t blocks = N * K / 32;
  if (blocks == 0) return;
  const int grid = (int)std::min<int64_t>((blocks + 255) / 256, 256 * 16);
  if (dtype == DT_BF16)
    w4_widen_kernel<bf16><<<grid, 256, 0, s>>>((bf16*)out, (const uint8_t*)W,
                                               (const uint8_t*)S, blocks);
  else
    w4_widen_kernel<f16><<<grid, 256, 0, s>>>((f16*)out, (const uint8_t*)W, (const uint8_t*)S,
                                              blocks);
}

}  // namespace kgc
