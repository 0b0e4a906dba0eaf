// K9q: weight-only FP8 (W8A16) skinny GEMM for small-batch decode on gfx950:
//   C[M, N] = (X[M, K] . W8[N, K]^T) * scale[N] (+ bias),  M <= 64,
// W8 the OCP e4m3 form of a linear layer's [out, in] weight with one fp32 scale per output
// row (ops/quant.py quantize_fp8_rows), X / C / bias bf16 or f16.
//
// The structure is K9's (gemm_skinny.hip): a workgroup owns 16*NT weight rows and ALL of K,
// its NW waves split K evenly, two register sets of loads are in flight, the per-wave
// partial sums merge in LDS and the workgroup writes coalesced rows of C.  What differs:
//   * the weight stream is half the bytes: a lane loads 16 consecutive e4m3 (one 16-byte
//     non-temporal load) and widens them in registers (common.h fp8x8_widen -- exact, every
//     e4m3 value is a bf16 and an f16) into the A operands of TWO v_mfma_f32_16x16x32: lane
//     (r16, q4) covers k = k0 + 16*q4 + [0, 8) in the first and + [8, 16) in the second.
//     The X fragments (B operand) are loaded with the same k-permutation -- 32 contiguous
//     bytes per lane -- and a permutation of k shared by A and B leaves the dot product
//     as it was.  One such pair of MFMAs is a "k-pair" (64 k) below;
//   * the MFMA runs on the unscaled e4m3 values; the epilogue is (sum of the NW partials)
//     * scale[n], then bias, then the one rounding -- the rounding points of K9;
//   * two epilogues only: plain, and W8_SILU over a merged [gate; up] weight [2I, K]
//     (n-tile 0 streams gate rows g0.., n-tile 1 the up rows I+g0.., each scaled by its own
//     channel scale): C[m, g] = silu(gate) * up, C [M, I].
// Shapes (checked on the host): N % (16*NT) == 0, K % (64*NW) == 0, 16-byte aligned rows.
//
// w8_widen: out[n, k] = round(W8[n, k] * scale[n]) in bf16 / f16 -- the M > 64 path widens
// a weight into a static scratch and runs the library GEMM on it.
#include "common.h"
#include "launch.h"

namespace kgc {

template <typename T, int MT, int NT, int NW, bool NTL, bool SILU>
__global__ __launch_bounds__(NW * 64) void w8_gemm_kernel(
    T* __restrict__ C, const T* __restrict__ X, const uint8_t* __restrict__ W,
    const float* __restrict__ scale, const T* __restrict__ bias, int M, int K, int64_t ldx,
    int64_t ldc) {
  static_assert(!SILU || NT == 2, "W8_SILU pairs n-tile 0 (gate) with n-tile 1 (up)");
  // k-pairs of loads in flight per register set (K9's U k-steps, two per pair); halved at
  // 16 waves, whose 1024 threads cap a lane at 128 VGPRs (the full sets spilled to scratch)
  constexpr int U = ((MT + NT) <= 2 ? 4 : 2) / (NW == 16 ? 2 : 1);
  __shared__ __attribute__((aligned(16))) float red[NW][MT][NT][64][4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r16 = lane & 15, q4 = lane >> 4;
  // W8_SILU: gridDim.x = I / 16 workgroups over the I = 16 * gridDim.x output columns
  const int64_t n0 = (int64_t)blockIdx.x * (SILU ? 16 : 16 * NT);
  const int64_t n_half = SILU ? (int64_t)gridDim.x * 16 : 0;
  const int kw = K / NW;
  const int kbeg = wave * kw, kend = kbeg + kw;

  const uint8_t* wrow[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
    wrow[nt] = W + (n0 + (SILU ? nt * n_half : 16 * nt) + r16) * (int64_t)K + 16 * q4;
  const T* xrow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) xrow[mt] = X + (int64_t)min(16 * mt + r16, M - 1) * ldx + 16 * q4;

  f32x4 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto ldw = [](const uint8_t* p) -> u32x4 {
    if constexpr (NTL) return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
    else return *reinterpret_cast<const u32x4*>(p);
  };
  // one k-pair: 16 e4m3 per weight row widened into two A fragments, two MFMAs per tile
  auto step = [&](const u32x4* wf, const Pack8<T> (*xf)[2]) {
    Pack8<T> a[NT][2];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      a[nt][0].u = fp8x8_widen<T>(u32x2{wf[nt].x, wf[nt].y});
      a[nt][1].u = fp8x8_widen<T>(u32x2{wf[nt].z, wf[nt].w});
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        acc[mt][nt] = mfma16x16x32(a[nt][0].v, xf[mt][0].v, acc[mt][nt]);
        acc[mt][nt] = mfma16x16x32(a[nt][1].v, xf[mt][1].v, acc[mt][nt]);
      }
  };

  typedef u32x4 WSet[U][NT];
  typedef Pack8<T> XSet[U][MT][2];
  auto load = [&](WSet& wf, XSet& xf, int k) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) wf[u][nt] = ldw(wrow[nt] + k + 64 * u);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        xf[u][mt][0].u = *reinterpret_cast<const u32x4*>(xrow[mt] + k + 64 * u);
        xf[u][mt][1].u = *reinterpret_cast<const u32x4*>(xrow[mt] + k + 64 * u + 8);
      }
  };
  auto compute = [&](const WSet& wf, const XSet& xf) {
#pragma unroll
    for (int u = 0; u < U; ++u) step(wf[u], xf[u]);
  };
  // two register sets (A, B): batch b+1's loads are in flight while batch b's MFMAs wait
  // only for their own (the compiler's wait-count pass places the counted waits)
  const int nb = (kend - kbeg) / (64 * U);
  auto kb = [&](int bi) { return kbeg + bi * 64 * U; };
  WSet wa, wb;
  XSet xa, xb;
  if (nb > 0) load(wa, xa, kb(0));
  for (int b = 0; b < nb; b += 2) {
    if (b + 1 < nb) load(wb, xb, kb(b + 1));
    compute(wa, xa);
    if (b + 1 < nb) {
      if (b + 2 < nb) load(wa, xa, kb(b + 2));
      compute(wb, xb);
    }
  }
  for (int k = kbeg + nb * 64 * U; k < kend; k += 64) {   // K-range not a multiple of 64*U
    u32x4 wf[NT];
    Pack8<T> xf[MT][2];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) wf[nt] = ldw(wrow[nt] + k);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      xf[mt][0].u = *reinterpret_cast<const u32x4*>(xrow[mt] + k);
      xf[mt][1].u = *reinterpret_cast<const u32x4*>(xrow[mt] + k + 8);
    }
    step(wf, xf);
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
    s *= scale[n0 + n];
    if constexpr (SILU) {
      float u = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) u += red[w][mt][1][l][i];
      u *= scale[n_half + n0 + n];
      C[(int64_t)m * ldc + n0 + n] = from_f<T>(s / (1.f + __expf(-s)) * u);
    } else {
      if (bias != nullptr) s += to_f<T>(bias[n0 + n]);
      C[(int64_t)m * ldc + n0 + n] = from_f<T>(s);
    }
  }
}

template <typename T, int MT, int NT, int NW>
static void w8_go(bool ntl, bool silu, dim3 grid, hipStream_t s, void* C, const void* X,
                  const void* W, const float* scale, const void* bias, int M, int K,
                  int64_t ldx, int64_t ldc) {
#define W8_GO(NTL_, SILU_)                                                              \
  w8_gemm_kernel<T, MT, NT, NW, NTL_, SILU_><<<grid, NW * 64, 0, s>>>(                  \
      (T*)C, (const T*)X, (const uint8_t*)W, scale, (const T*)bias, M, K, ldx, ldc)
  if constexpr (NT == 2) {
    if (silu) {
      if (ntl) W8_GO(true, true);
      else W8_GO(false, true);
      return;
    }
  }
  if (ntl) W8_GO(true, false);
  else W8_GO(false, false);
#undef W8_GO
}

template <typename T, int MT>
static void w8_mt(int nt, int nw, bool ntl, bool silu, void* C, const void* X, const void* W,
                  const float* scale, const void* bias, int M, int N, int K, int64_t ldx,
                  int64_t ldc, hipStream_t s) {
  const dim3 grid(silu ? N / 32 : N / (16 * nt));   // silu: N = 2I
#define W8_NW(NT_, NW_) \
  w8_go<T, MT, NT_, NW_>(ntl, silu, grid, s, C, X, W, scale, bias, M, K, ldx, ldc)
  if (nt == 2) {
    // (mt, nt, nw) = (4, 2, 16) does not exist: 32 accumulators + one load set exceed the
    // 128 VGPRs of a 1024-thread workgroup (it spilled); the host checks reject it
    if (nw == 16) {
      if constexpr (MT < 4) W8_NW(2, 16);
    } else if (nw == 8) W8_NW(2, 8);
    else W8_NW(2, 4);
  } else {
    if (nw == 16) W8_NW(1, 16);
    else if (nw == 8) W8_NW(1, 8);
    else W8_NW(1, 4);
  }
#undef W8_NW
}

template <typename T>
static void w8_t(int mt, int nt, int nw, bool ntl, bool silu, void* C, const void* X,
                 const void* W, const float* scale, const void* bias, int M, int N, int K,
                 int64_t ldx, int64_t ldc, hipStream_t s) {
  if (mt == 1) w8_mt<T, 1>(nt, nw, ntl, silu, C, X, W, scale, bias, M, N, K, ldx, ldc, s);
  else if (mt == 2) w8_mt<T, 2>(nt, nw, ntl, silu, C, X, W, scale, bias, M, N, K, ldx, ldc, s);
  else w8_mt<T, 4>(nt, nw, ntl, silu, C, X, W, scale, bias, M, N, K, ldx, ldc, s);
}

void launch_w8_gemm(int dtype, int mt, int nt, int nw, bool ntl, bool silu, void* C,
                    const void* X, const void* W, const float* scale, const void* bias, int M,
                    int N, int K, int64_t ldx, int64_t ldc, hipStream_t s) {
  if (M == 0 || N == 0) return;
  if (dtype == DT_BF16)
    w8_t<bf16>(mt, nt, nw, ntl, silu, C, X, W, scale, bias, M, N, K, ldx, ldc, s);
  else
    w8_t<f16>(mt, nt, nw, ntl, silu, C, X, W, scale, bias, M, N, K, ldx, ldc, s);
}

// ---- w8_widen: 16 e4m3 per thread -> 16 T, scaled by the row's scale and rounded once
template <typename T>
__global__ __launch_bounds__(256) void w8_widen_kernel(T* __restrict__ out,
                                                       const uint8_t* __restrict__ W,
                                                       const float* __restrict__ scale,
                                                       int64_t chunks, int chunks_per_row) {
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < chunks;
       c += (int64_t)gridDim.x * 256) {
    const float sc = scale[c / chunks_per_row];
    const u32x4 raw = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(W + c * 16));
    const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
    Pack8<T> o[2];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8(w[j], false);
      const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8(w[j], true);
      // the fp32 products exist as such (as in the K9q epilogue and on the CPU): otherwise
      // the f16 form may fuse product and conversion into one v_fma_mix rounding
      float p[4] = {lo[0] * sc, lo[1] * sc, hi[0] * sc, hi[1] * sc};
      asm("" : "+v"(p[0]), "+v"(p[1]), "+v"(p[2]), "+v"(p[3]));
      T* h = &o[j >> 1].h[4 * (j & 1)];
#pragma unroll
      for (int e = 0; e < 4; ++e) h[e] = from_f<T>(p[e]);
    }
    u32x4* dst = reinterpret_cast<u32x4*>(out + c * 16);
    dst[0] = o[0].u;
    dst[1] = o[1].u;
  }
}

void launch_w8_widen(int dtype, void* out, const void* W, const float* scale, int64_t N,
                     int64_t K, hipStream_t s) {
  const int64_t chunks = N * K / 16;
  if (chunks == 0) return;
  const int grid = (int)std::min<int64_t>((chunks + 255) / 256, 256 * 16);
  if (dtype == DT_BF16)
    w8_widen_kernel<bf16><<<grid, 256, 0, s>>>((bf16*)out, (const uint8_t*)W, scale, chunks,
                                               (int)(K / 16));
  else
    w8_widen_kernel<f16><<<grid, 256, 0, s>>>((f16*)out, (const uint8_t*)W, scale, chunks,
                                              (int)(K / 16));
}

}  // namespace kgc
