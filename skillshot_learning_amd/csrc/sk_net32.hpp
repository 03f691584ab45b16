// sk_net32.hpp — what the two halves of the fp32 learner share: the size
// constants and flat parameter offsets of the nets, the Net views and the
// launder helpers, the 10-round Philox, the TP32 trace hooks, the MFMA
// fragments (the split-bf16 32-row GEMMs mfb / mf6 / gemm6, the 16-row f32
// ones m16* / g16_* / w1_frag), the DPP row sums, the LDS-only barrier and
// the host's set_lds32.
//
// Included by sk_act32.hpp (the acting half) and sk_learn32.hip (the gradient
// half), which are one translation unit: everything here sits in the
// anonymous namespace, as the kernels built on it do, so this is not a header
// to share between translation units.
//
// MFMA operand layout of the 32-row tiles.  v_mfma_f32_32x32x2_f32 contracts
// K = 2: lane l holds A[l%32][k0 + l/32] and B[k0 + l/32][l%32]; D register v
// of lane l is D[8(v/4) + 4(l/32) + v%4][l%32] (drow).  The bf16 MFMAs that
// replaced it in the acting tile (gemm6) keep that D layout.
#ifndef SK_NET32_HPP
#define SK_NET32_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sk_mlp.hpp"
#include "sk_partial.hpp"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));  // W2 rows of the critic are 8-B aligned

constexpr int kIn = 12, kH1 = 256, kH2 = 128;
constexpr int kLdH1 = 260, kLdH2 = 132;  // LDS row strides (floats): 16-B aligned, banks rotated
constexpr int kThreads = 512;                        // grad kernels: 8 waves per 32-row sub-tile
constexpr int kFwdThreads = 256;                     // forward: 4 waves per 32-row tile

// flat parameter offsets (torch parameters() order)
constexpr int kPW1 = 0, kPB1 = kH1 * kIn, kPW2 = kPB1 + kH1;
__host__ __device__ constexpr int pB2(int ld2) { return kPW2 + kH2 * ld2; }
__host__ __device__ constexpr int pW3(int ld2) { return pB2(ld2) + kH2; }
__host__ __device__ constexpr int pB3(int ld2, int n_out) { return pW3(ld2) + n_out * kH2; }
constexpr int kCLd = kH1 + 2, kALd = kH1;
constexpr int kCP = pB3(kCLd, 1) + 1, kAP = pB3(kALd, 2) + 2;
static_assert(kCP == 36609 && kAP == 36482 && kCP == skpart::kCriticParams && kPW2 == skpart::kPW2, "parameter counts");

// Weights are read through GLOBAL-address-space pointers: laundered (below)
// generic pointers would become FLAT loads, which count on lgkmcnt too, so
// every LDS wait would also wait for the in-flight weight loads
typedef const __attribute__((address_space(1))) float* gfp;
typedef const __attribute__((address_space(1))) f4u* gf4u;
struct Net {  // views into one flat parameter vector
  gfp W1, b1, W2, b2, W3, b3;
  int ld2;
};
__device__ __forceinline__ Net net_of(const float* f, int ld2, int n_out) {
  const gfp g = (gfp)f;
  return Net{g + kPW1, g + kPB1, g + kPW2, g + pB2(ld2), g + pW3(ld2), g + pB3(ld2, n_out), ld2};
}

// Re-derive a net's bases (and the lane id) inside a sub-tile loop: without
// this LICM hoists every per-lane load address out of the loop and spills
// them (the same trap as sk_update.hip's fragment loads)
__device__ __forceinline__ const float* launder(const float* base) {
  asm volatile("" : "+s"(base));  // one SGPR pair per net; the parameter offsets are immediates
  return base;
}
__device__ __forceinline__ int launder_lane(int lane) {
  asm volatile("" : "+v"(lane));
  return lane;
}

__device__ __forceinline__ int drow(int v, int lane) { return 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3); }

__device__ __forceinline__ uint4 philox(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint64_t p0 = (uint64_t)c.x * 0xD2511F53u, p1 = (uint64_t)c.z * 0xCD9E8D57u;  // v_mad_u64_u32
    c = make_uint4(__builtin_amdgcn_bitop3_b32((uint32_t)(p1 >> 32), c.y, k0, 0x96), (uint32_t)p1,
                   __builtin_amdgcn_bitop3_b32((uint32_t)(p0 >> 32), c.w, k1, 0x96), (uint32_t)p0);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

// Phase timestamps of the first and last workgroup (diagnostic builds only:
// -DSK_TRACE32, read back with sk_debug_trace32; tools/trace_learn32.py)
#ifdef SK_TRACE32
__device__ unsigned long long g_sk_trace32[2][32][2];
#define TP32(k)                                                                              \
  do {                                                                                       \
    if (threadIdx.x == 0 && (blockIdx.x == 0 || blockIdx.x == gridDim.x - 1)) {              \
      const int wg_ = blockIdx.x == 0 ? 0 : 1;                                               \
      g_sk_trace32[wg_][k][0] = __builtin_amdgcn_s_memtime();                                \
      g_sk_trace32[wg_][k][1] = wall_clock64();                                              \
    }                                                                                        \
  } while (0)
#else
#define TP32(k) \
  do {          \
  } while (0)
#endif

// ------------------------------------------------------------------ the acting tile's GEMMs
// fp32 products from bf16 pieces (sk_split.hpp): D[i][n] += sum_k X[i][k]
// W[n][k] as six v_mfma_f32_32x32x16_bf16 per 16 k — the small piece
// products first, the hi x hi last — into one fp32 accumulator; the
// variance GEMM of parameter noise (x^2 W^2, which only scales the noise) is
// one more on bf16 squares.  A = the activations, row-major bf16 planes in
// LDS (hi, mid, lo, square: `xp` elements apart), lane (r, h) reading row r,
// k = 16 kk + 8 h + 0..7 (16 bytes); B = the weights' split pack in global
// memory (fragment order, planes `wp` elements apart), one 16-byte load per
// lane and k-step.  D register v of lane l is D[8(v/4) + 4(l/32) + v%4][l%32],
// the layout of the f32 MFMA these replace: every epilogue is unchanged.
typedef const __attribute__((address_space(1))) skmlp::bf16x8* gbf8;
using skmlp::bf16x8;
__device__ __forceinline__ f32x16 mfb(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mf6(const bf16x8 x[3], const bf16x8 w[3], f32x16 m) {
  m = mfb(x[2], w[0], m);
  m = mfb(x[0], w[2], m);
  m = mfb(x[1], w[1], m);
  m = mfb(x[1], w[0], m);
  m = mfb(x[0], w[1], m);
  return mfb(x[0], w[0], m);
}
// kk k-steps of the tile: X rows at X (row stride ldx elements), W fragments
// of n-tile `frag0` (kk-th at frag0 + 64 kk lanes); VAR adds the variance GEMM
template <int KK, bool VAR>
__device__ __forceinline__ void gemm6(f32x16& m, f32x16& v, const short* X, int ldx, int xp, gbf8 W, int wp,
                                      int lane) {
  const int i = lane & 31, h = lane >> 5;
  const short* xr = X + i * ldx + 8 * h;
  gbf8 wr = W + lane;
  constexpr int NP = VAR ? 4 : 3;
  bf16x8 wn[2][NP];  // two k-steps of weight fragments in flight
#pragma unroll
  for (int d = 0; d < 2 && d < KK; ++d)
#pragma unroll
    for (int q = 0; q < NP; ++q) wn[d][q] = wr[(size_t)q * (wp / 8) + 64 * d];
#pragma unroll
  for (int kk = 0; kk < KK; ++kk) {
    bf16x8 wc[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) wc[q] = wn[kk & 1][q];
    if (kk + 2 < KK) {
#pragma unroll
      for (int q = 0; q < NP; ++q) wn[kk & 1][q] = wr[(size_t)q * (wp / 8) + 64 * (kk + 2)];
    }
    bf16x8 x[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) x[q] = *(const bf16x8*)(xr + q * xp + 16 * kk);
    m = mf6(x, wc, m);
    if (VAR) v = mfb(x[3], wc[3], v);
  }
}

// ------------------------------------------------------------------ 16-row f32 fragments
// The gradient kernels and the 16-row actor forward work on 16-row sub-tiles
// on v_mfma_f32_16x16x4_f32 (the fp32 MFMA rate is the bound: a 16-row
// sub-tile per workgroup spreads a minibatch over twice the CUs of 32-row
// tiles).  Lane l = (i = l % 16, g = l / 16): A[i][k = g],
// B[k = g][i], D register r = D[4g + r][i] (4 consecutive rows of column i).
// The float4 trick of the 32x32 GEMMs: lane (i, g) loads k0 + 4g .. + 3 and
// MFMA t contracts {k0 + t, k0 + 4 + t, k0 + 8 + t, k0 + 12 + t}.
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kR = 16;                         // rows per sub-tile
constexpr int kLdS16 = 20, kLdT16 = 20;        // [16][20] states; transposed [unit][16 rows (+4)]

__device__ __forceinline__ f32x4 m16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 m16x4(f4 a, f4 b, f32x4 c) {
  c = m16(a.x, b.x, c);
  c = m16(a.y, b.y, c);
  c = m16(a.z, b.z, c);
  return m16(a.w, b.w, c);
}

// layer 1 (K = 12): k 0..11 by lane groups 0-2 (group 3's 12..15 are zero
// operands: S is zero-padded, W1 is not read)
__device__ __forceinline__ f32x4 g16_l1(const float* S, gfp W1, int n0, int lane) {
  const int i = lane & 15, g = lane >> 4;
  const f4 x = *(const f4*)(S + i * kLdS16 + 4 * g);
  f4 w = {0.f, 0.f, 0.f, 0.f};
  if (g < 3) w = *(gf4u)(W1 + (n0 + i) * kIn + 4 * g);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  return m16x4(x, w, acc);
}
// D[row][n0 + j] = sum_k X[row][k] W[n0 + j][k] over the 256 inputs (X in
// LDS [16][ldx], W global row-major), for one net (a) or two nets' chains
// interleaved (b); the weight loads of the next 4 steps are in flight
__device__ __forceinline__ f32x4 g16_xwT256(const float* X, int ldx, gfp W, int ldw, int n0, int lane) {
  const int i = lane & 15, g = lane >> 4;
  const float* xr = X + i * ldx + 4 * g;
  const gfp wr = W + (size_t)(n0 + i) * ldw + 4 * g;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  f4 wn[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) wn[t] = *(gf4u)(wr + 16 * t);
#pragma unroll
  for (int k = 0; k < 256; k += 64) {
    f4 wc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) wc[t] = wn[t];
    if (k + 64 < 256) {
#pragma unroll
      for (int t = 0; t < 4; ++t) wn[t] = *(gf4u)(wr + k + 64 + 16 * t);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) acc = m16x4(*(const f4*)(xr + k + 16 * t), wc[t], acc);
  }
  return acc;
}
__device__ __forceinline__ void g16_xwT256x2(f32x4& a0, f32x4& a1, const float* X0, gfp W0, int ldw0, const float* X1,
                                             gfp W1, int ldw1, int n0, int lane) {
  const int i = lane & 15, g = lane >> 4;
  const float* x0 = X0 + i * kLdH1 + 4 * g;
  const float* x1 = X1 + i * kLdH1 + 4 * g;
  const gfp w0 = W0 + (size_t)(n0 + i) * ldw0 + 4 * g;
  const gfp w1 = W1 + (size_t)(n0 + i) * ldw1 + 4 * g;
  a0 = f32x4{0.f, 0.f, 0.f, 0.f};
  a1 = f32x4{0.f, 0.f, 0.f, 0.f};
  f4 n0w[2], n1w[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    n0w[t] = *(gf4u)(w0 + 16 * t);
    n1w[t] = *(gf4u)(w1 + 16 * t);
  }
#pragma unroll
  for (int k = 0; k < 256; k += 32) {
    f4 c0[2], c1[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      c0[t] = n0w[t];
      c1[t] = n1w[t];
    }
    if (k + 32 < 256) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        n0w[t] = *(gf4u)(w0 + k + 32 + 16 * t);
        n1w[t] = *(gf4u)(w1 + k + 32 + 16 * t);
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      a0 = m16x4(*(const f4*)(x0 + k + 16 * t), c0[t], a0);
      a1 = m16x4(*(const f4*)(x1 + k + 16 * t), c1[t], a1);
    }
  }
}
// D[row][n0 + j] = sum_{u < 128} DZ[row][u] W[u][n0 + j]: DZ in LDS [16][ldz],
// W global row-major read down its columns (16 lanes: 64 contiguous bytes)
__device__ __forceinline__ f32x4 g16_xw128(const float* DZ, int ldz, gfp W, int ldw, int n0, int lane) {
  const int i = lane & 15, g = lane >> 4;
  const float* zr = DZ + i * ldz + 4 * g;
  const gfp wc = W + (size_t)(4 * g) * ldw + n0 + i;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  f4 bn[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
    bn[t] = f4{wc[(16 * t + 0) * ldw], wc[(16 * t + 1) * ldw], wc[(16 * t + 2) * ldw], wc[(16 * t + 3) * ldw]};
#pragma unroll
  for (int k = 0; k < 128; k += 64) {
    f4 bc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) bc[t] = bn[t];
    if (k + 64 < 128) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int r = k + 64 + 16 * t;
        bn[t] = f4{wc[(r + 0) * ldw], wc[(r + 1) * ldw], wc[(r + 2) * ldw], wc[(r + 3) * ldw]};
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) acc = m16x4(*(const f4*)(zr + k + 16 * t), bc[t], acc);
  }
  return acc;
}
// weight gradient of one 16 x 16 tile over the sub-tile's 16 rows: acc[m][n]
// += sum_row AT[m0 + m][row] BT[n0 + n][row] (both transposed in LDS)
__device__ __forceinline__ f32x4 g16_wgrad(f32x4 acc, const float* AT, int m0, const float* BT, int n0, int lane) {
  const int i = lane & 15, g = lane >> 4;
  return m16x4(*(const f4*)(AT + (m0 + i) * kLdT16 + 4 * g), *(const f4*)(BT + (n0 + i) * kLdT16 + 4 * g), acc);
}

// inclusive prefix sum over the 16 lanes of a DPP row (row_shr 1, 2, 4, 8,
// zero fill): lane 15 of each row holds the row's total
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float rowsum16(float v) {
  v += dpp_f<0x111>(v);
  v += dpp_f<0x112>(v);
  v += dpp_f<0x114>(v);
  v += dpp_f<0x118>(v);
  return v;
}

// LDS-only workgroup barrier (outstanding global loads stay in flight)
__device__ __forceinline__ void lds_sync32() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// g16_l1's weight fragment of unit n0 + i on its own, for callers that issue
// it ahead of their staging barrier (an unconditional load, zeroed by select
// where g = 3: the conditional load's phi cost the actor's backward a
// vmcnt(0) right after it)
__device__ __forceinline__ f4 w1_frag(gfp W1, int n0, int lane) {
  const int i = lane & 15, g = lane >> 4;
  const f4 v = *(gf4u)(W1 + (n0 + i) * kIn + 4 * (g < 3 ? g : 0));
  const bool ok = g < 3;
  return f4{ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f};
}

// host: a kernel's dynamic LDS above the 64 KiB default
template <typename K>
void set_lds32(K kernel, size_t bytes) {
  (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace

#endif  // SK_NET32_HPP
