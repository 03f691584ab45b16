// sk_act32.hpp — the acting half of the fp32 learner: the actor forward at
// the reference's precision and every kernel that plays the game with it.
//
//   k_actor_fwd32    actor forward 12 -> 256 relu -> 128 relu -> 2 tanh for a
//                    [rows, 12] batch on 32-row tiles (actor_tile32: fp32
//                    products from split bf16 pieces, sk_split.hpp), optionally
//                    with the reference's parameter noise w <- w (1 + sd
//                    N(0,1)) (SkillshotLearner.py:245-281) sampled exactly in
//                    distribution per row by local reparameterisation, and
//                    action noise
//   k_actor_fwd16    the same forward on 16-row f32 tiles (actor_tile16): the
//                    default up to 4,096 rows
//   k_act_step32     the self-play tick: act + step (+ ring insert) in one
//                    launch; act_step32, its body, is also the acting part of
//                    k_bwd_act_step32 (sk_learn32.hip)
//   k_act_episode32  every game's whole episode in one launch, then
//   k_episode_finish the counters' advance by the ticks played
//   k_act_match32    two actors play whole matches in one launch
//   k_act_league32   every pairing of K actors in one launch
//   k_act_match32_rec, k_act_league32_rec  the same two, keeping each tick's
//                    state, actions and rewards of the first games of every
//                    block (the match record)
//   k_act_step_pool32  the opponent-pool training tick: each block of games
//                    acts from the two actors its pairing names, one of them
//                    the noisy learner, then steps and inserts as k_act_step32
//   k_act_league32_bots, k_act_step_pool32_bots  the league (plain and
//                    recording) and the pool tick where a seat may be a
//                    scripted actor (csrc/sk_bot.hpp): no tile for that seat
//   k_act_league32_stats  the league (plain and recording, nets and scripted
//                    actors alike) tallying each seat's match statistics
//                    (csrc/sk_stats.hpp) in wave 0's registers
//   k_split_pack32   the actor's split pack from its flat fp32 parameters
// and, at the end, their host launchers (sk_launch_act_*, declared in
// sk_step.hpp and called by sk_engine.hip and sk_learn32.hip) and C entry
// points (sk_actor_forward_f32, sk_actor_split_pack_*).
//
// Part of sk_learn32.hip's translation unit, not a header to share: the
// kernels sit in the anonymous namespace and keep their names, so
// sk_learn32.hip includes this file once; k_bwd_act_step32 there joins
// act_step32 with the sliced backward.
#ifndef SK_ACT32_HPP
#define SK_ACT32_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/skillshot.h"
#include "sk_mlp.hpp"
#include "sk_net32.hpp"
#include "sk_split.hpp"
#include "sk_stats.hpp"
#include "sk_step.hpp"

namespace {

// ---------------------------------------------------------------- actor forward
// the last workgroup to arrive stores the call number the launch drew with.
// Grouped arrival (as the bf16 actor's advance_call, csrc/sk_actor.hip):
// workgroup b on group line call_ctr[2 + 16 (b % 8)], the last of each group
// on call_ctr[1] (SK_ACTOR_COUNTER_WORDS); nb = the launch's workgroups that
// arrive (the first nb of the grid)
__device__ __forceinline__ void advance_call32(uint64_t* call_ctr, uint64_t call, unsigned nb) {
  if (threadIdx.x == 0) {
    const unsigned g = blockIdx.x & 7u;
    const unsigned long long members = (nb - g + 7u) / 8u;
    unsigned long long* gc = (unsigned long long*)&call_ctr[2 + 16 * g];
    if (atomicAdd(gc, 1ull) == members - 1) {
      *gc = 0;
      const unsigned long long groups = nb < 8u ? nb : 8u;
      if (atomicAdd((unsigned long long*)&call_ctr[1], 1ull) == groups - 1) {
        call_ctr[0] = call;
        call_ctr[1] = 0;
      }
    }
  }
}
// mean and variance GEMMs of parameter noise on 16-row tiles (g16_xwT256 with
// x^2 w^2 beside: every operand load feeds both chains)
__device__ __forceinline__ void g16_xwT256_mv(f32x4& m, f32x4& v, const float* X, gfp W, int n0, int lane) {
  const int i = lane & 15, g = lane >> 4;
  const float* xr = X + i * kLdH1 + 4 * g;
  const gfp wr = W + (size_t)(n0 + i) * kALd + 4 * g;
  m = f32x4{0.f, 0.f, 0.f, 0.f};
  v = f32x4{0.f, 0.f, 0.f, 0.f};
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
    for (int t = 0; t < 4; ++t) {
      const f4 x = *(const f4*)(xr + k + 16 * t);
      m = m16x4(x, wc[t], m);
      v = m16x4(x * x, wc[t] * wc[t], v);
    }
  }
}

// 4 normals for the rows r .. r+3 of unit `unit` of `layer` (Box-Muller on
// the 4 Philox words: two pairs)
__device__ __forceinline__ void normals4(uint64_t seed, uint64_t call, uint32_t r, uint32_t layer_unit, float z[4]) {
  const uint4 u = philox(make_uint4(r, layer_unit, (uint32_t)call, (uint32_t)(call >> 32)), (uint32_t)seed,
                         (uint32_t)(seed >> 32));
  const uint32_t wd[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const float u1 = ((float)(wd[2 * q] >> 8) + 0.5f) * 0x1p-24f;  // (0, 1)
    const float u2 = (float)(wd[2 * q + 1] >> 8) * 0x1p-24f;       // [0, 1)
    const float rad = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1));  // -2 ln u1
    z[2 * q] = rad * __builtin_amdgcn_cosf(u2);  // v_cos_f32 / v_sin_f32 take revolutions
    z[2 * q + 1] = rad * __builtin_amdgcn_sinf(u2);
  }
}

// 4 noisy pre-activations of rows r .. r+3 of unit `layer_unit`:
// y = m + b + sd sqrt(b^2 + v) xi, the xi keyed as normals4's (the same
// Philox counter, 24-bit uniforms, Box-Muller in revolutions) but in pair
// form: sqrt((b^2 + v) L) with L = -2 ln(u1) sd^2 carries the radius, one
// square root per element instead of the radius's plus the element's, and
// Philox4x32 with kF32NoiseRounds rounds (7: the fewest BigCrush-passing
// rounds, as the bf16 path's noise; sk_mlp.hpp).  k2 = noise_k2(sd).
constexpr int kF32NoiseRounds = 7;
// noisy4 in two parts, bit for bit the same: the draws (Philox words ->
// the pairs' L and cos / sin; independent of the GEMM) and the combination
// with m and v.  actor_tile32 draws layer 2's noise after its second half's
// GEMM.  Drawing it before that GEMM, under its MFMAs, was measured and
// dropped: neutral at two workgroups per CU
// (profiles/r04g_noise_hoist_ab.jsonl); at three its 24 live registers
// spilled (config 5 acting 119 vs 112 us, profiles/r04p_hoist_ab.jsonl)
struct Draw4 {
  float L[2], c[2], s[2];
};
__device__ __forceinline__ Draw4 draw4n(uint64_t seed, uint64_t call, uint32_t r, uint32_t layer_unit, float k2) {
  const uint4 u = skmlp::philox<kF32NoiseRounds>(
      make_uint4(r, layer_unit, (uint32_t)call, (uint32_t)(call >> 32)), (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint32_t wd[4] = {u.x, u.y, u.z, u.w};
  Draw4 d;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const float u1 = ((float)(wd[2 * q] >> 8) + 0.5f) * 0x1p-24f;  // (0, 1)
    const float u2 = (float)(wd[2 * q + 1] >> 8) * 0x1p-24f;       // [0, 1) revolutions
    d.L[q] = k2 * __builtin_amdgcn_logf(u1);                        // -2 ln(u1) sd^2
    d.c[q] = __builtin_amdgcn_cosf(u2);
    d.s[q] = __builtin_amdgcn_sinf(u2);
  }
  return d;
}
template <typename V>
__device__ __forceinline__ void noisy4_apply(const Draw4& d, float b, const V& m, const V& v, int o, float y[4]) {
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    y[2 * q] = __builtin_fmaf(__builtin_amdgcn_sqrtf(__builtin_fmaf(b, b, v[o + 2 * q]) * d.L[q]), d.c[q],
                              m[o + 2 * q] + b);
    y[2 * q + 1] = __builtin_fmaf(__builtin_amdgcn_sqrtf(__builtin_fmaf(b, b, v[o + 2 * q + 1]) * d.L[q]), d.s[q],
                                  m[o + 2 * q + 1] + b);
  }
}
template <typename V>
__device__ __forceinline__ void noisy4(uint64_t seed, uint64_t call, uint32_t r, uint32_t layer_unit, float k2,
                                       float b, const V& m, const V& v, int o, float y[4]) {
  const uint4 u = skmlp::philox<kF32NoiseRounds>(
      make_uint4(r, layer_unit, (uint32_t)call, (uint32_t)(call >> 32)), (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint32_t wd[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const float u1 = ((float)(wd[2 * q] >> 8) + 0.5f) * 0x1p-24f;  // (0, 1)
    const float u2 = (float)(wd[2 * q + 1] >> 8) * 0x1p-24f;       // [0, 1) revolutions
    const float L = k2 * __builtin_amdgcn_logf(u1);                 // -2 ln(u1) sd^2
    const float c = __builtin_amdgcn_cosf(u2), s = __builtin_amdgcn_sinf(u2);
    y[2 * q] = __builtin_fmaf(__builtin_amdgcn_sqrtf(__builtin_fmaf(b, b, v[o + 2 * q]) * L), c, m[o + 2 * q] + b);
    y[2 * q + 1] =
        __builtin_fmaf(__builtin_amdgcn_sqrtf(__builtin_fmaf(b, b, v[o + 2 * q + 1]) * L), s, m[o + 2 * q + 1] + b);
  }
}

// Row maps of a 32-row actor tile: local row i -> global row of the [rows]
// batch, and whether it exists.  Contiguous: rows row0 .. row0 + 31.
// Players (the self-play tick, k_act_step32): games g0 .. g0 + 15, rows
// g0 + i (player 1) and N + g0 + i - 16 (player 2) of the actor's
// player-major [2N] order.  Parameter / action noise is keyed by the global
// row (the first row of an aligned 4-row group), so with N % 4 == 0 both maps
// draw the same noise for the same row.
struct RowsContig {
  static constexpr bool kStore = true;  // the tile writes its actions to `out` (compile time)
  int64_t row0, rows;
  __device__ int64_t operator()(int i) const { return row0 + i; }
  __device__ bool valid(int i) const { return row0 + i < rows; }
};
struct RowsPlayers {
  static constexpr bool kStore = true;
  int64_t g0, n;
  __device__ int64_t operator()(int i) const { return i < 16 ? g0 + i : n + g0 + (i - 16); }
  __device__ bool valid(int i) const { return g0 + (i & 15) < n; }
};
// One seat of a match (k_act_match32): the 32 rows of player `seat` of games
// g0 .. g0 + 31, rows seat N + g0 + i.  The actions stay in LDS (no global
// store: float2 rows of player 2 would sit at 8 N bytes, and nobody reads them).
struct RowsSeat {
  static constexpr bool kStore = false;
  int64_t base, g0, n;  // base = seat N
  __device__ int64_t operator()(int i) const { return base + g0 + i; }
  __device__ bool valid(int i) const { return g0 + i < n; }
};
// The same seat where the actions are wanted in `out` as well (the pool tick,
// k_act_step_pool32: actions float[2N][2] as sk_env_act_step writes them).
// With N % 32 == 0 every aligned 4-row group of a seat's rows is one of the
// contiguous map's, so the noise drawn for a row is k_actor_fwd32's.
struct RowsSeatStore : RowsSeat {
  static constexpr bool kStore = true;
};

// one 32-row tile per workgroup of 4 waves: layer 1 n-tiles w, 4 + w,
// layer 2 n-tile w, layer 3 by all threads.  NOISE: per layer y = xW + b +
// sd sqrt(x^2 W^2 + b^2) xi, xi ~ N(0,1) per (row, unit) (exact in
// distribution for w' = w (1 + sd N(0,1)) drawn per row, each noisy weight
// being used once per row).  The actions go to out[R(i)] and, if act_lds,
// to act_lds[i].  GEMMs on split bf16 pieces (gemm6, sk_split.hpp): fp32
// products at the bf16 MFMA rate, W1 / W2 read from the actor's split pack
// `pk`, biases and W3 from the flat vector.  LDS (ActorLds, kActorTileLds
// bytes): the observations and the layer-1 outputs as four bf16 planes each
// (hi, mid, lo, square; written once by the producing lane, read by every
// wave's A fragments), layer 2's fp32 outputs over the layer-1 planes once
// every wave has read them.  Round 3's f32-MFMA tile (128 dependent 32x32x2
// f32 MFMAs per wave in layer 2: 5.2 us of the 4,096-game acting launch,
// profiles/r03t_*) and its variance GEMM's bf16 operands are replaced.
// Layer 1 runs in two halves of 128 units (n-tile 4h + w per wave), each
// followed by its 8 k-steps of layer 2 into the same accumulators (the k
// order, hence every sum, of one 16-step chain): the planes hold one half,
// 41 KB of LDS per tile instead of 74 KB, so three workgroups share a CU
// instead of two.
// waves per SIMD the acting kernels are compiled for (their VGPR budget:
// 512 / waves): with the half-size planes three workgroups share a CU
// (config 5 acting 127 -> 112 us; at two waves, 185
// VGPRs, no gain: profiles/r04o_act_waves_ab.jsonl).  The episode kernel at
// two: it held every loop-invariant weight fragment of the tile across the
// episode (512 VGPRs, one workgroup per CU, spills) until its weight
// addresses were made opaque per tick (180 -> 110 us per tick,
// profiles/r04o_episode_ab.jsonl).  The pool tick at two: with a noisy and
// a plain tile behind a branch and wave 0's step lanes live across both it
// spills 136 VGPRs at three waves and 26 at two (the compiler's resource
// report)
constexpr int kActWaves = 3, kEpisodeWaves = 2, kPoolWaves = 2;
constexpr int kLdX1 = 24, kLdX2 = 136;              // bf16 row strides (48 / 272 B: conflict-free 16-B reads)
constexpr int kX1Plane = 32 * kLdX1, kX2Plane = 32 * kLdX2;  // kX2Plane: one half of layer 1's units
constexpr size_t kActorTileLds = (size_t)(4 * kX1Plane + 4 * kX2Plane) * 2;
static_assert((size_t)32 * kLdH2 * 4 <= (size_t)4 * kX2Plane * 2, "layer 2's outputs fit over the layer-1 planes");
struct ActorLds {
  short* S;   // [4 planes][32][kLdX1]
  short* H1;  // [4 planes][32][kLdX2]
  float* H2;  // [32][kLdH2], aliasing H1
};
__device__ __forceinline__ ActorLds actor_lds(char* base) {
  ActorLds L;
  L.S = (short*)base;
  L.H1 = L.S + 4 * kX1Plane;
  L.H2 = (float*)L.H1;
  return L;
}
// the four planes of element (row, col) of a bf16-plane block
__device__ __forceinline__ void put4(short* P, int plane, int at, float v) {
  short hi, mid, lo, sq;
  sksplit::split4(v, hi, mid, lo, sq);
  P[at] = hi;
  P[plane + at] = mid;
  P[2 * plane + at] = lo;
  P[3 * plane + at] = sq;
}

template <bool NOISE, typename MAP>
__device__ __forceinline__ void actor_tile32(const Net& A, const char* __restrict__ pk,
                                             const float* __restrict__ X, float* __restrict__ out, const MAP& R,
                                             float sd, float action_sd, uint64_t seed, uint64_t call, ActorLds T,
                                             float2* act_lds) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int t = threadIdx.x; t < 32 * 16; t += kFwdThreads) {  // S[i][k] = obs (k < 12, valid rows), else 0
    const int i = t >> 4, k = t & 15;
    put4(T.S, kX1Plane, i * kLdX1 + k, (k < kIn && R.valid(i)) ? X[R(i) * kIn + k] : 0.f);
  }
  __syncthreads();
  TP32(2);
  const gbf8 W1 = (gbf8)(pk + sksplit::kOffW1), W2 = (gbf8)(pk + sksplit::kOffW2);
  const int u2 = 32 * w + (lane & 31);  // this wave's layer-2 unit
  const float k2 = skmlp::noise_k2(sd);
  Draw4 dr[4];
  f32x16 m2 = {0}, var2 = {0};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    {  // layer 1, units 128 h .. 128 h + 127: n-tile 4 h + w, into the planes' column u - 128 h
      const int nt = 4 * h + w, u = 32 * nt + (lane & 31), col = u - 128 * h;
      f32x16 m = {0}, var = {0};
      gemm6<1, NOISE>(m, var, T.S, kLdX1, kX1Plane, W1 + 64 * nt, sksplit::kW1Plane, lane);
      const float b = A.b1[u];
      if (NOISE) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float y[4];
          noisy4(seed, call, (uint32_t)R(drow(4 * g, lane)), (uint32_t)u, k2, b, m, var, 4 * g, y);
#pragma unroll
          for (int q = 0; q < 4; ++q) put4(T.H1, kX2Plane, drow(4 * g + q, lane) * kLdX2 + col, fmaxf(y[q], 0.f));
        }
      } else {
#pragma unroll
        for (int v = 0; v < 16; ++v) put4(T.H1, kX2Plane, drow(v, lane) * kLdX2 + col, fmaxf(m[v] + b, 0.f));
      }
    }
    __syncthreads();
    if (h == 0) TP32(3);
    // layer 2, k = 128 h .. 128 h + 127 (k-steps 8 h .. 8 h + 7 of n-tile w)
    gemm6<8, NOISE>(m2, var2, T.H1, kLdX2, kX2Plane, W2 + 16 * 64 * w + 8 * 64 * h, sksplit::kW2Plane, lane);
    __syncthreads();  // every wave has read this half: the next half / layer 2's outputs go over it
  }
  {
    const float b = A.b2[u2];
    if (NOISE) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float y[4];
        dr[g] = draw4n(seed, call, (uint32_t)R(drow(4 * g, lane)), (uint32_t)(kH1 + u2), k2);
        noisy4_apply(dr[g], b, m2, var2, 4 * g, y);
#pragma unroll
        for (int q = 0; q < 4; ++q) T.H2[drow(4 * g + q, lane) * kLdH2 + u2] = fmaxf(y[q], 0.f);
      }
    } else {
#pragma unroll
      for (int v = 0; v < 16; ++v) T.H2[drow(v, lane) * kLdH2 + u2] = fmaxf(m2[v] + b, 0.f);
    }
  }
  __syncthreads();
  TP32(4);
  {  // layer 3: thread t -> row t / 8, units 16 (t % 8) .. (both outputs)
    const float* H2 = T.H2;
    const int i = threadIdx.x >> 3, c = threadIdx.x & 7;
    float m0 = 0.f, m1 = 0.f, v0 = 0.f, v1 = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int u = 16 * c + k;
      const float h = H2[i * kLdH2 + u], w0 = A.W3[u], w1 = A.W3[kH2 + u];
      m0 += h * w0;
      m1 += h * w1;
      if (NOISE) {
        v0 += h * h * w0 * w0;
        v1 += h * h * w1 * w1;
      }
    }
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) {
      m0 += __shfl_xor(m0, off, 64);
      m1 += __shfl_xor(m1, off, 64);
      if (NOISE) {
        v0 += __shfl_xor(v0, off, 64);
        v1 += __shfl_xor(v1, off, 64);
      }
    }
    if (c == 0 && R.valid(i)) {
      const int64_t row = R(i);
      float y0 = m0 + A.b3[0], y1 = m1 + A.b3[1];
      if (NOISE) {
        float z[4];
        normals4(seed, call, (uint32_t)row, (uint32_t)(kH1 + kH2), z);
        y0 += sd * __builtin_amdgcn_sqrtf(v0 + A.b3[0] * A.b3[0]) * z[0];
        y1 += sd * __builtin_amdgcn_sqrtf(v1 + A.b3[1] * A.b3[1]) * z[1];
      }
      float o0 = tanhf(y0), o1 = tanhf(y1);
      if (action_sd != 0.f) {  // model_act_action_noise (:229-243): tanh output + N(0, sd), unclipped
        float z[4];
        normals4(seed, call, (uint32_t)row, (uint32_t)(kH1 + kH2 + 1), z);
        o0 += action_sd * z[0];
        o1 += action_sd * z[1];
      }
      if (MAP::kStore) *(float2*)(out + row * 2) = make_float2(o0, o1);
      if (act_lds) act_lds[i] = make_float2(o0, o1);
    }
  }
}

template <bool NOISE>
__global__ void __launch_bounds__(kFwdThreads, kActWaves) k_actor_fwd32(const float* __restrict__ aflat,
                                                             const char* __restrict__ apack,
                                                             const float* __restrict__ X, float* __restrict__ out,
                                                             int64_t rows, float sd, float action_sd, uint64_t seed,
                                                             uint64_t* __restrict__ call_ctr) {
  extern __shared__ __attribute__((aligned(16))) float smem_sl[];
  const Net A = net_of(aflat, kALd, 2);
  // a launch that draws noise (parameter or action) uses call number
  // counter + 1 and its last workgroup stores that number back
  const bool draws = (NOISE || action_sd != 0.f) && call_ctr;
  const uint64_t call = draws ? call_ctr[0] + 1 : 0;
  actor_tile32<NOISE>(A, apack, X, out, RowsContig{(int64_t)blockIdx.x * 32, rows}, sd, action_sd, seed, call,
                      actor_lds((char*)smem_sl), nullptr);
  if (draws) {  // the last workgroup to finish stores the call number it drew with
    __syncthreads();
    advance_call32(call_ctr, call, gridDim.x);
  }
}

// The self-play tick's act + step in ONE launch (VERDICT r02 item 3;
// SkillshotLearner.py:304-314 act -> do_actions -> game_tick -> get_state,
// with the replay ring insert of sk_env_step_insert): workgroup b owns games
// 16b .. 16b + 15.  Wave 0's lanes 0-31 issue k_step_split's state loads
// (both players of the 16 games) first, so they land under the actor's
// MFMA chain; the 4 waves run the fp32 actor tile on the games' 32
// observation rows (RowsPlayers); the actions meet in LDS; wave 0 then
// finishes k_step_split's tick for its lanes.  Equal, bit for bit, to
// sk_actor_forward_f32 (32-row tiles) followed by sk_env_step(_insert).
// Wave 0 counts its games into counter slot line b.
// act_step32: the body on the LDS at `smem` (the actor tile's, then sAct)
// for the first nb workgroups of the grid (k_act_step32: all of them;
// k_bwd_act_step32: the workgroups before the backward's)
constexpr size_t kActStepLds = kActorTileLds + 32 * sizeof(float2);
template <bool NOISE>
__device__ __forceinline__ void act_step32(const float* __restrict__ aflat, const char* __restrict__ apack,
                                           float* __restrict__ act_out, float sd, float action_sd, uint64_t seed,
                                           uint64_t* __restrict__ call_ctr, sk::StepArgs a, sk::Cfg c, char* smem,
                                           unsigned nb) {
  float2* sAct = (float2*)(smem + kActorTileLds);
  const int lane = threadIdx.x & 63;
  const bool w0 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) == 0;
  const int64_t g0 = (int64_t)blockIdx.x * 16;
  sk_counters* slot = a.ctr ? a.ctr + (size_t)blockIdx.x * SK_CTR_STRIDE : nullptr;
  TP32(0);
  sk::StepLane L;
  if (w0) L = sk::split_load(a, lane < 32 ? 2 * g0 + lane : 2 * a.n, slot);
  TP32(1);
  const Net A = net_of(aflat, kALd, 2);
  const bool draws = (NOISE || action_sd != 0.f) && call_ctr;
  const uint64_t call = draws ? call_ctr[0] + 1 : 0;
  actor_tile32<NOISE>(A, apack, a.acting_obs, act_out, RowsPlayers{g0, a.n}, sd, action_sd, seed, call,
                      actor_lds(smem), sAct);
  TP32(5);
  __syncthreads();
  TP32(6);
  if (w0) {
    const float2 act = lane < 32 ? sAct[(lane & 1) * 16 + (lane >> 1)] : make_float2(0.f, 0.f);
    sk::split_finish(a, c, L, act, slot);
  }
  TP32(7);
  if (draws) {
    __syncthreads();
    advance_call32(call_ctr, call, nb);
  }
}

template <bool NOISE>
__global__ void __launch_bounds__(kFwdThreads, kActWaves) k_act_step32(const float* __restrict__ aflat,
                                                            const char* __restrict__ apack,
                                                            float* __restrict__ act_out, float sd, float action_sd,
                                                            uint64_t seed, uint64_t* __restrict__ call_ctr,
                                                            sk::StepArgs a, sk::Cfg c) {
  extern __shared__ __attribute__((aligned(16))) float smem_sl[];
  act_step32<NOISE>(aflat, apack, act_out, sd, action_sd, seed, call_ctr, a, c, (char*)smem_sl, gridDim.x);
}


// The reference rule's episode collection (model_train, SkillshotLearner.py
// :289-318) in ONE launch: every game plays its episode
// from the current state, act (the actor held fixed for the epoch, fresh
// exploration noise per tick: tick t draws with call number call0 + 1 + t,
// as t sk_env_act_step calls would) -> do_actions -> game_tick -> get_state
// while game_live and ticks < tick_limit (:304); a game that has ended is
// stepped no further, as the reference's loop stops.  Workgroup b owns
// games 16b .. 16b + 15 for the whole episode (act_step32's geometry: no
// workgroup waits for another) and leaves once all of them have ended.
// Tick t reads the acting states at states[t] ([2][N][12], player-major;
// states[0] is the caller's observation of the start) and writes the
// actions to actions[t] ([2][N][2]), the post-tick observation to
// states[t + 1] and the reward to rewards[t] ([2][N]); lengths[i] = the
// ticks game i played.  The rows t < lengths[i] of both players are the
// episode's (s, a, r) for models_fit (:320-357); later rows are undefined.  The step counter and the
// noise call number advance by the ticks the per-tick loop would have run,
// max_i lengths[i] (it had been n_ticks, so the next epoch's
// restarts and noise diverged from the loop's whenever every game ended
// before the limit): k_episode_finish, one workgroup launched after this
// kernel on the same stream, reduces the lengths and stores both.
struct EpisodeArgs {
  float* states;
  float* actions;
  float* rewards;
  int32_t* lengths;
  int n_ticks;
};
template <bool NOISE>
__global__ void __launch_bounds__(kFwdThreads, kEpisodeWaves) k_act_episode32(const float* __restrict__ aflat,
                                                               const char* __restrict__ apack, float sd,
                                                               float action_sd, uint64_t seed,
                                                               uint64_t* __restrict__ call_ctr, sk::StepArgs a,
                                                               sk::Cfg c, EpisodeArgs ep) {
  extern __shared__ __attribute__((aligned(16))) float smem_sl[];
  char* smem = (char*)smem_sl;
  float2* sAct = (float2*)(smem + kActorTileLds);
  int* sAlive = (int*)(sAct + 32);
  const int lane = threadIdx.x & 63;
  const bool w0 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) == 0;
  const int64_t g0 = (int64_t)blockIdx.x * 16;
  // no episode counters: a lane whose game has ended skips split_finish's
  // count, and the slot line is stored by lane 0 (the episode's outcome is
  // the final state and `lengths`)
  sk_counters* const slot = nullptr;
  const bool draws = (NOISE || action_sd != 0.f) && call_ctr;
  const uint64_t call0 = draws ? call_ctr[0] : 0;
  const int64_t n = a.n, gt = 2 * g0 + lane, gi = gt >> 1;  // wave 0: lane -> (game, player)
  if (w0 && lane < 32 && (lane & 1) == 0 && gi < n) ep.lengths[gi] = 0;
  for (int t = 0; t < ep.n_ticks; ++t) {
    // the weights' addresses opaque per tick: otherwise every weight fragment
    // and bias the tile loads is loop-invariant, hoisted out of the loop and
    // held (or spilled) across the whole episode
    const float* af = aflat;
    const char* pk = apack;
    asm volatile("" : "+s"(af), "+s"(pk));
    const Net A = net_of(af, kALd, 2);
    sk::StepArgs at = a;
    at.acting_obs = ep.states + (int64_t)t * 24 * n;
    at.obs = ep.states + (int64_t)(t + 1) * 24 * n;
    at.reward = ep.rewards + (int64_t)t * 2 * n;
    sk::StepLane L;
    // the state loads fly under the actor tile (act_step32's order); the
    // loop test waits for them only after it
    if (w0) L = sk::split_load(at, lane < 32 ? gt : 2 * n, slot);
    actor_tile32<NOISE>(A, pk, at.acting_obs, ep.actions + (int64_t)t * 4 * n, RowsPlayers{g0, n}, sd,
                        action_sd, seed, call0 + 1 + (uint64_t)t, actor_lds(smem), sAct);
    if (w0) {
      // the reference's loop test (:304) on the pre-tick state; both lanes of a game agree
      const bool alive = L.in && ((L.mi.y >> 16) & 0xff) && L.mi.x < a.tick_limit;
      L.in = alive;  // an ended game is neither stepped nor written
      if (alive && L.p == 0) ep.lengths[L.i] = t + 1;
      const uint64_t any = __ballot(alive);
      if (lane == 0) *sAlive = any != 0;
    }
    __syncthreads();
    if (!*sAlive) break;  // workgroup-uniform: every game of the workgroup has ended
    if (w0) {
      const float2 act = lane < 32 ? sAct[(lane & 1) * 16 + (lane >> 1)] : make_float2(0.f, 0.f);
      sk::split_finish(at, c, L, act, slot);
    }
    __syncthreads();  // this tick's observations are the next tick's acting rows (this workgroup's own stores)
  }
}

// The episode's counter advance (see k_act_episode32): T = max lengths[i]
// (the per-tick loop's iterations: it runs while any game lives), then the
// step slot step0 + T and, when the episode drew, the call number call0 + T.
// Both start values are read here: the episode kernel leaves the counters
// alone, and this launch follows it on the stream.
__global__ void __launch_bounds__(256) k_episode_finish(const int32_t* __restrict__ lengths, int64_t n,
                                                        sk::StepRef step, uint64_t* __restrict__ call_ctr) {
  __shared__ int red[4];
  int m = 0;
  for (int64_t i = threadIdx.x; i < n; i += 256) m = max(m, lengths[i]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = max(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint64_t T = (uint64_t)max(max(red[0], red[1]), max(red[2], red[3]));
    step.slots[1 - step.parity] = step.slots[step.parity] + T;
    if (call_ctr) call_ctr[0] = call_ctr[0] + T;
  }
}

// Head-to-head evaluation (sk_env_act_match): two actors play whole matches
// in ONE launch, seat 1 (player id 1) acting from net 1 and seat 2 from net
// 2, without noise (SkillshotLearner.py:302-318 with two policies).  The
// self-play tile (RowsPlayers) puts both players of 16 games in one MFMA tile,
// so both share every weight fragment; here workgroup b owns the 32 games
// 32b .. 32b + 31 and runs the tile twice per tick: the 32 player-1 rows
// through net 1 (actions -> sAct[0..31]), the 32 player-2 rows through net 2
// (-> sAct[32..63]).  Wave 0's 64 lanes are the (game, player) lanes of
// k_step_split: split_load before the tiles (the state loads fly under both
// MFMA chains), the episode kernel's loop test, split_finish after them.
// LDS between the tiles: tile 1's layer 3 reads H2; tile 2 first writes S
// (disjoint: tile 1's last S read, layer 1 of its second half, lies three
// barriers back) and writes H1 (aliasing H2) only after its first
// __syncthreads(), which every thread reaches after its layer 3 of tile 1.
// sAct is read by wave 0 after the barrier that follows tile 2, and tile 1 of
// tick t + 1 starts after the closing barrier of tick t.
// Observations ping-pong in obs2 [2][2][N][12]: tick t reads half t & 1 and
// writes half (t + 1) & 1 (this workgroup's own stores, ordered by the
// closing barrier); no trajectory is recorded.  returns [2][N] (nullable) is
// in/out: each (player, game) lane adds, in fp32 and in tick order, the
// rewards of the ticks it played onto the value it found, so a match played
// in several launches sums as one launch does.  split_finish stores the
// tick's reward into the lane's own returns element, the lane reads it back
// (its own store) and writes the sum at the end.  Counters: k_episode_finish
// after this kernel, as for the episode (the step counter advances by
// max_i lengths[i]); neither actor's noise call number is touched.
struct MatchArgs {
  float* obs2;
  float* returns;
  int32_t* lengths;
  int32_t* last_half;
  int n_ticks;
};
constexpr size_t kActMatchLds = kActorTileLds + 64 * sizeof(float2) + 16;
// The match record (sk_env_act_match_rec / sk_env_act_league_rec, DESIGN
// §18): the recording instantiations (REC) keep, for the first per_block
// games of every block of games, each tick's pre-tick state, both seats'
// actions and rewards, and the state after the game's last tick of the call.
// Game k < per_block of block b is row j = b per_block + k; state (s, j) lies
// at index s rows + j of each plane (the engine's layout, `rows` games per
// slab), the action and the reward of seat p + 1 at tick t at [(slab0 + t) 2
// + p] rows + j.  A game that plays c >= 1 ticks of the call writes slabs
// slab0 .. slab0 + c of its row and nothing past them; one that plays none
// writes nothing.  The pre-tick state is what split_load just loaded, the
// action what the lane hands to split_finish, the reward what the lane reads
// back for its return: plain vector stores of values already in registers.
struct RecArgs {
  int2* pos;
  double* rot;
  int2* qpos;
  double* qrot;
  int2* qcdage;
  int2* misc;
  float* actions;   // [slabs - 1][2][rows][2]
  float* rewards;   // [slabs - 1][2][rows] (nullable)
  int64_t rows;
  int per_block, slab0;
  int wgs_per_block;  // the league's block / 32 (a match is one block of N games: unused)
};
// one state of a recorded row: this (game, player) lane's half of the five
// player planes, and misc from the player-1 lane
__device__ __forceinline__ void rec_state(const RecArgs& rc, int64_t at, int p, int2 pp, double rot, int2 qq,
                                          double qrot, int2 ca, int2 mi) {
  const int64_t h = 2 * at + p;
  rc.pos[h] = pp;
  rc.rot[h] = rot;
  rc.qpos[h] = qq;
  rc.qrot[h] = qrot;
  rc.qcdage[h] = ca;
  if (p == 0) rc.misc[at] = mi;
}
// match_ticks32: a workgroup's matches from the first tick to the last, on
// the LDS at `smem` (kActMatchLds bytes).  k_act_match32 runs it on its
// arguments, k_act_league32 on the two actors its pairing names.  REC (the
// _rec kernels): the workgroup's games are games rec_k0 .. rec_k0 + 31 of
// block rec_b of the record `rc`; every line of it is under if constexpr.
// BOTS (the _bots kernels): seat s + 1 is the scripted actor of kind
// kind<s + 1> when that is non-zero (workgroup-uniform: it follows from the
// pairing).  Such a seat runs no tile; wave 0's lanes of that seat compute
// the policy (sk::bot_lane) on what split_load loaded and the partner lane's
// position, at step L.step + t (the launch's step value is the same at every
// tick; the per-tick loop's counter has advanced by t), and store it into
// sAct where the tile would have, ahead of the barrier wave 0 reads sAct
// behind.  With both seats scripted waves 1-3 only keep the barriers.  Every
// line of it is under if constexpr as well.
// STAT (the _stats kernel): wave 0's (game, player) lanes keep the seat's
// eight statistics (csrc/sk_stats.hpp) and its previous position in registers,
// update them right behind the loop test from what split_load loaded and the
// partner lane's position and projectile (the pair exchange, as bot_lane's),
// and store the eight words once after the loop, into stats int32
// [SK_N_STATS + 2][2][N]: a lane whose game lived no tick of the call (a pad
// game among them) stores nothing.  Every line of it is under if constexpr.
template <bool REC, bool BOTS = false, bool STAT = false>
__device__ __forceinline__ void match_ticks32(const float* aflat1, const char* apack1, const float* aflat2,
                                              const char* apack2, const sk::StepArgs& a, const sk::Cfg& c,
                                              const MatchArgs& mt, char* smem, const RecArgs* rc = nullptr,
                                              int rec_b = 0, int rec_k0 = 0, int kind1 = 0, int kind2 = 0,
                                              int32_t* stats = nullptr) {
  float2* sAct = (float2*)(smem + kActorTileLds);
  int* sAlive = (int*)(sAct + 64);
  const int lane = threadIdx.x & 63;
  const bool w0 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) == 0;
  const int64_t g0 = (int64_t)blockIdx.x * 32;
  sk_counters* const slot = nullptr;  // no episode counters (see k_act_episode32)
  const int64_t n = a.n, gt = 2 * g0 + lane, gi = gt >> 1;  // wave 0: lane -> (game, player)
  const bool mine = w0 && gi < n;
  float* const ret = mine && mt.returns ? mt.returns + (int64_t)(lane & 1) * n + gi : nullptr;
  float acc = ret ? *ret : 0.f;
  if (mine && (lane & 1) == 0) mt.lengths[gi] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0 && mt.last_half) *mt.last_half = mt.n_ticks & 1;
  // the record: whether the workgroup records at all is uniform (its first
  // game's k), whether a lane does is its own k; rec_live = the lane's game
  // played the tick before (its row then takes the state found at this one)
  bool rec_wg = false, rec_lane = false, rec_live = false;
  int64_t rec_j = 0;
  if constexpr (REC) {
    rec_wg = w0 && rec_k0 < rc->per_block;
    rec_lane = mine && rec_k0 + (lane >> 1) < rc->per_block;
    rec_j = (int64_t)rec_b * rc->per_block + rec_k0 + (lane >> 1);
  }
  int32_t sv[SK_N_STATS] = {0, 0, 0, 0, 0, 0, 0, skstat::kFar}, sxp = skstat::kNoPrev, syp = 0;  // STAT only
  for (int t = 0; t < mt.n_ticks; ++t) {
    // both nets' addresses opaque per tick (k_act_episode32's reason, twice over)
    const float *af1 = aflat1, *af2 = aflat2;
    const char *pk1 = apack1, *pk2 = apack2;
    asm volatile("" : "+s"(af1), "+s"(pk1), "+s"(af2), "+s"(pk2));
    sk::StepArgs at = a;
    at.acting_obs = mt.obs2 + (int64_t)(t & 1) * 24 * n;
    at.obs = mt.obs2 + (int64_t)((t + 1) & 1) * 24 * n;
    at.reward = mt.returns;
    sk::StepLane L;
    if (w0) L = sk::split_load(at, gt, slot);  // lanes past the tail: in = false
    if constexpr (BOTS) {
      if (!kind1)
        actor_tile32<false>(net_of(af1, kALd, 2), pk1, at.acting_obs, nullptr, RowsSeat{0, g0, n}, 0.f, 0.f, 0, 0,
                            actor_lds(smem), sAct);
      if (!kind2)
        actor_tile32<false>(net_of(af2, kALd, 2), pk2, at.acting_obs, nullptr, RowsSeat{n, g0, n}, 0.f, 0.f, 0, 0,
                            actor_lds(smem), sAct + 32);
      if (w0 && (kind1 | kind2)) {
        const int kind = (lane & 1) ? kind2 : kind1;
        const float2 b = sk::bot_lane(kind, lane & 1, L.pp, L.rot, c, a.seed, (uint64_t)(a.env_offset + L.ic),
                                      L.step + (uint64_t)t);
        if (kind) sAct[(lane & 1) * 32 + (lane >> 1)] = b;
      }
    } else {
      actor_tile32<false>(net_of(af1, kALd, 2), pk1, at.acting_obs, nullptr, RowsSeat{0, g0, n}, 0.f, 0.f, 0, 0,
                          actor_lds(smem), sAct);
      actor_tile32<false>(net_of(af2, kALd, 2), pk2, at.acting_obs, nullptr, RowsSeat{n, g0, n}, 0.f, 0.f, 0, 0,
                          actor_lds(smem), sAct + 32);
    }
    if (w0) {
      // the reference's loop test (:304) on the pre-tick state; both lanes of a game agree
      const bool alive = L.in && ((L.mi.y >> 16) & 0xff) && L.mi.x < a.tick_limit;
      L.in = alive;  // an ended game (a league's pad game from the start) is neither stepped nor written
      if (alive && L.p == 0) mt.lengths[L.i] = t + 1;
      const uint64_t any = __ballot(alive);
      if (lane == 0) *sAlive = any != 0;
      if constexpr (REC) {
        // slab slab0 + t: the pre-tick state of a game that plays tick t, or
        // the final state of one that played tick t - 1 and is found ended
        if (rec_wg) {
          if (rec_lane && (alive || rec_live))
            rec_state(*rc, (int64_t)(rc->slab0 + t) * rc->rows + rec_j, L.p, L.pp, L.rot, L.qq, L.qrot, L.ca, L.mi);
          rec_live = alive;
        }
      }
      if constexpr (STAT) {
        // the partner lane's position and projectile: every lane of wave 0 takes part in the exchange
        const int ox = sk::pair_swap(L.pp.x), oy = sk::pair_swap(L.pp.y);
        const int oqx = sk::pair_swap(L.qq.x), oqy = sk::pair_swap(L.qq.y);
        if (alive) {
          const sktrig::SinCos m = skbot::sincos(L.rot, [](double x) { return sk::sincos_lib(x); });
          const unsigned f = (unsigned)L.mi.y;
          skstat::tick(sv, sxp, syp, m, L.pp.x, L.pp.y, ox, oy, L.ca.x, ((f >> (8 * L.p)) & 0xff) != 0,
                       ((f >> (8 * (1 - L.p))) & 0xff) != 0, oqx, oqy, c.psize, c.pspeed, c.W, c.H);
        }
      }
    }
    __syncthreads();
    if (!*sAlive) break;  // workgroup-uniform: every game of the workgroup has ended
    if (w0) {
      const float2 act = sAct[(lane & 1) * 32 + (lane >> 1)];
      sk::split_finish(at, c, L, act, slot);
      float r = 0.f;
      if (L.in && ret) acc += r = *ret;  // the reward split_finish just stored for this (player, game)
      if constexpr (REC) {
        if (rec_wg && rec_lane && L.in) {
          const int64_t at_a = ((int64_t)(rc->slab0 + t) * 2 + L.p) * rc->rows + rec_j;
          rc->actions[2 * at_a] = act.x;
          rc->actions[2 * at_a + 1] = act.y;
          if (rc->rewards && ret) rc->rewards[at_a] = r;
        }
      }
    }
    __syncthreads();  // this tick's observations are the next tick's acting rows (this workgroup's own stores)
  }
  if (ret) *ret = acc;
  if constexpr (STAT) {
    if (mine && sxp != skstat::kNoPrev) {  // gi < n: plane k, seat lane & 1, game gi
#pragma unroll
      for (int k = 0; k < SK_N_STATS; ++k) stats[((int64_t)k * 2 + (lane & 1)) * n + gi] = sv[k];
    }
  }
  if constexpr (REC) {
    // a game still playing when n_ticks ran out (a break leaves rec_live
    // false in every lane): its state after the last tick, slab slab0 +
    // n_ticks, is the lane's own plane stores read back
    if (rec_wg && rec_lane && rec_live) {
      const int p = lane & 1;
      const int64_t h = gt;
      rec_state(*rc, (int64_t)(rc->slab0 + mt.n_ticks) * rc->rows + rec_j, p, reinterpret_cast<const int2*>(a.v.pos)[h],
                reinterpret_cast<const double*>(a.v.rot)[h], reinterpret_cast<const int2*>(a.v.qpos)[h],
                reinterpret_cast<const double*>(a.v.qrot)[h], reinterpret_cast<const int2*>(a.v.qcdage)[h],
                a.v.misc[gi]);
    }
  }
}
__global__ void __launch_bounds__(kFwdThreads, kEpisodeWaves) k_act_match32(const float* __restrict__ aflat1,
                                                                            const char* __restrict__ apack1,
                                                                            const float* __restrict__ aflat2,
                                                                            const char* __restrict__ apack2,
                                                                            sk::StepArgs a, sk::Cfg c, MatchArgs mt) {
  extern __shared__ __attribute__((aligned(16))) float smem_sl[];
  match_ticks32<false>(aflat1, apack1, aflat2, apack2, a, c, mt, (char*)smem_sl);
}
// k_act_match32 keeping a record: the match is one block of N games, so
// workgroup b's games are k = 32b .. 32b + 31 of block 0
__global__ void __launch_bounds__(kFwdThreads, kEpisodeWaves) k_act_match32_rec(const float* __restrict__ aflat1,
                                                                                const char* __restrict__ apack1,
                                                                                const float* __restrict__ aflat2,
                                                                                const char* __restrict__ apack2,
                                                                                sk::StepArgs a, sk::Cfg c, MatchArgs mt,
                                                                                RecArgs rc) {
  extern __shared__ __attribute__((aligned(16))) float smem_sl[];
  match_ticks32<true>(aflat1, apack1, aflat2, apack2, a, c, mt, (char*)smem_sl, &rc, 0, (int)blockIdx.x * 32);
}

// League evaluation (sk_env_act_league): every ordered pairing of K actors
// in ONE launch.  The env holds P blocks of `block` games (a multiple of 32),
// pairing p owns games p block .. (p + 1) block - 1, and workgroup b, which
// owns games 32b .. 32b + 31 as in k_act_match32, plays pairing b / (block /
// 32): it reads pairs[p] = (seat-1 actor, seat-2 actor) and those actors'
// rows of nets = (flat vector, split pack) once, with uniform (scalar)
// loads, and from there on is k_act_match32's workgroup, the four addresses
// opaque per tick: it calls match_ticks32, the loop k_act_match32 runs.
// Sharing the loop compiled both kernels to other code than their two
// separate copies had (233 VGPRs and 126 SGPR spills each, against 234 and
// 138), measured no slower.  A pairing whose games are no
// multiple of 32 is padded by the caller with games whose live byte is 0:
// the loop test never steps or writes them and their lengths stay 0.  A
// pair index outside [0, K), a null address or one the tile cannot load
// from (flat 4-byte, pack 16-byte aligned) is not followed: the workgroup
// writes lengths = 0 for its games, touches nothing else and returns.
struct LeagueArgs {
  const uint64_t* nets;  // [K][2]
  const int32_t* pairs;  // [P][2]
  int n_actors;
  int wgs_per_pair;      // block / 32
};
__global__ void __launch_bounds__(kFwdThreads, kEpisodeWaves) k_act_league32(LeagueArgs lg, sk::StepArgs a,
                                                                                sk::Cfg c, MatchArgs mt) {
  extern __shared__ __attribute__((aligned(16))) float smem_sl[];
  const int p = (int)blockIdx.x / lg.wgs_per_pair;
  const int i1 = lg.pairs[2 * p], i2 = lg.pairs[2 * p + 1];
  uint64_t f1 = 0, k1 = 0, f2 = 0, k2 = 0;
  if ((unsigned)i1 < (unsigned)lg.n_actors && (unsigned)i2 < (unsigned)lg.n_actors) {
    f1 = lg.nets[2 * i1];
    k1 = lg.nets[2 * i1 + 1];
    f2 = lg.nets[2 * i2];
    k2 = lg.nets[2 * i2 + 1];
  }
  if (!f1 || !k1 || !f2 || !k2 || ((f1 | f2) & 3) || ((k1 | k2) & 15)) {
    const int64_t g = (int64_t)blockIdx.x * 32 + threadIdx.x;
    if (threadIdx.x < 32 && g < a.n) mt.lengths[g] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0 && mt.last_half) *mt.last_half = mt.n_ticks & 1;
    return;
  }
  match_ticks32<false>((const float*)f1, (const char*)k1, (const float*)f2, (const char*)k2, a, c, mt,
                       (char*)smem_sl);
}
// k_act_league32 keeping a record: its prologue and guard line for line (a
// shared wrapper compiled the plain kernel's guard to other code, so each
// keeps its own); pairing p is block p of the record and the workgroup's
// first game is game 32 (blockIdx.x - p wgs_per_block) of it, both scalar.  A
// pairing the guard refuses records nothing.
__global__ void __launch_bounds__(kFwdThreads, kEpisodeWaves) k_act_league32_rec(LeagueArgs lg, sk::StepArgs a,
                                                                                    sk::Cfg c, MatchArgs mt,
                                                                                    RecArgs rc) {
  extern __shared__ __attribute__((aligned(16))) float smem_sl[];
  const int p = (int)blockIdx.x / lg.wgs_per_pair;
  const int i1 = lg.pairs[2 * p], i2 = lg.pairs[2 * p + 1];
  uint64_t f1 = 0, k1 = 0, f2 = 0, k2 = 0;
  if ((unsigned)i1 < (unsigned)lg.n_actors && (unsigned)i2 < (unsigned)lg.n_actors) {
    f1 = lg.nets[2 * i1];
    k1 = lg.nets[2 * i1 + 1];
    f2 = lg.nets[2 * i2];
    k2 = lg.nets[2 * i2 + 1];
  }
  if (!f1 || !k1 || !f2 || !k2 || ((f1 | f2) & 3) || ((k1 | k2) & 15)) {
    const int64_t g = (int64_t)blockIdx.x * 32 + threadIdx.x;
    if (threadIdx.x < 32 && g < a.n) mt.lengths[g] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0 && mt.last_half) *mt.last_half = mt.n_ticks & 1;
    return;
  }
  match_ticks32<true>((const float*)f1, (const char*)k1, (const float*)f2, (const char*)k2, a, c, mt, (char*)smem_sl,
                      &rc, p, ((int)blockIdx.x - p * rc.wgs_per_block) * 32);
}
// A league with scripted actors among its seats (sk_env_act_league_bots /
// _bots_rec): k_act_league32's workgroup, where a row of nets whose first
// word is 0 and whose second is a kind code in [1, 4] is a scripted actor
// (include/skillshot.h, csrc/sk_bot.hpp) and every other row a net under the
// guard above.  A kernel of its own, so that the net-only kernels keep their
// code; one template for the plain and the recording form (REC false: rc is
// not read).
__device__ __forceinline__ int bot_kind(uint64_t flat, uint64_t word) {
  return (!flat && word >= (uint64_t)SK_BOT_STILL && word <= (uint64_t)SK_BOT_CHASER) ? (int)word : 0;
}
__device__ __forceinline__ bool net_ok(uint64_t flat, uint64_t pack) {
  return flat && pack && !(flat & 3) && !(pack & 15);
}
template <bool REC>
__global__ void __launch_bounds__(kFwdThreads, kEpisodeWaves) k_act_league32_bots(LeagueArgs lg, sk::StepArgs a,
                                                                                     sk::Cfg c, MatchArgs mt,
                                                                                     RecArgs rc) {
  extern __shared__ __attribute__((aligned(16))) float smem_sl[];
  const int p = (int)blockIdx.x / lg.wgs_per_pair;
  const int i1 = lg.pairs[2 * p], i2 = lg.pairs[2 * p + 1];
  uint64_t f1 = 0, k1 = 0, f2 = 0, k2 = 0;
  if ((unsigned)i1 < (unsigned)lg.n_actors && (unsigned)i2 < (unsigned)lg.n_actors) {
    f1 = lg.nets[2 * i1];
    k1 = lg.nets[2 * i1 + 1];
    f2 = lg.nets[2 * i2];
    k2 = lg.nets[2 * i2 + 1];
  }
  const int b1 = bot_kind(f1, k1), b2 = bot_kind(f2, k2);
  if (!(b1 || net_ok(f1, k1)) || !(b2 || net_ok(f2, k2))) {
    const int64_t g = (int64_t)blockIdx.x * 32 + threadIdx.x;
    if (threadIdx.x < 32 && g < a.n) mt.lengths[g] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0 && mt.last_half) *mt.last_half = mt.n_ticks & 1;
    return;
  }
  match_ticks32<REC, true>((const float*)f1, (const char*)k1, (const float*)f2, (const char*)k2, a, c, mt,
                           (char*)smem_sl, &rc, p, ((int)blockIdx.x - p * lg.wgs_per_pair) * 32, b1, b2);
}
// The league with the statistics tallied in the launch
// (sk_env_act_league_stats): k_act_league32_bots' prologue and guard line for
// line, then match_ticks32<REC, true, true>.  A kernel of its own, so that a
// call without statistics keeps the kernels it had.  A pairing the guard
// refuses stores no statistics.
template <bool REC>
__global__ void __launch_bounds__(kFwdThreads, kEpisodeWaves) k_act_league32_stats(LeagueArgs lg, sk::StepArgs a,
                                                                                      sk::Cfg c, MatchArgs mt,
                                                                                      RecArgs rc, int32_t* stats) {
  extern __shared__ __attribute__((aligned(16))) float smem_sl[];
  const int p = (int)blockIdx.x / lg.wgs_per_pair;
  const int i1 = lg.pairs[2 * p], i2 = lg.pairs[2 * p + 1];
  uint64_t f1 = 0, k1 = 0, f2 = 0, k2 = 0;
  if ((unsigned)i1 < (unsigned)lg.n_actors && (unsigned)i2 < (unsigned)lg.n_actors) {
    f1 = lg.nets[2 * i1];
    k1 = lg.nets[2 * i1 + 1];
    f2 = lg.nets[2 * i2];
    k2 = lg.nets[2 * i2 + 1];
  }
  const int b1 = bot_kind(f1, k1), b2 = bot_kind(f2, k2);
  if (!(b1 || net_ok(f1, k1)) || !(b2 || net_ok(f2, k2))) {
    const int64_t g = (int64_t)blockIdx.x * 32 + threadIdx.x;
    if (threadIdx.x < 32 && g < a.n) mt.lengths[g] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0 && mt.last_half) *mt.last_half = mt.n_ticks & 1;
    return;
  }
  match_ticks32<REC, true, true>((const float*)f1, (const char*)k1, (const float*)f2, (const char*)k2, a, c, mt,
                                 (char*)smem_sl, &rc, p, ((int)blockIdx.x - p * lg.wgs_per_pair) * 32, b1, b2, stats);
}

// The opponent-pool training tick (sk_env_act_step_pool): k_act_step32's tick
// with k_act_league32's seating.  Workgroup b owns games 32b .. 32b + 31 and
// plays pairing p = b / (block / 32): pairs[p] and those actors' rows of nets
// are read once with uniform loads, under the league's guard.  One tick per
// launch: split_load for wave 0's 64 (game, player) lanes first (the state
// and ring-source loads fly under both MFMA chains), the tile on the 32
// seat-1 rows from net pairs[p][0], the tile on the 32 seat-2 rows from net
// pairs[p][1] (RowsSeatStore: actions to `act_out` and to sAct), then
// split_finish with the caller's full StepArgs: obs, reward, done, winner,
// auto-reset, obs_reset, the ring insert, the episode counters into slot
// line b.  A seat draws noise iff its actor is `noisy_actor`: parameter
// noise through actor_tile32<true> when sd != 0, action noise by action_sd,
// both with call number call_ctr[0] + 1 and keyed by the global row of the
// [2N] order; every other seat is actor_tile32<false> with action_sd 0.
// Whether a seat is noisy is workgroup-uniform; the seat loop is kept rolled
// so the kernel holds one inlined tile of each kind.  LDS between the two
// tiles: as match_ticks32's.  The launch advances the call number once
// (advance_call32 over the whole grid) iff it was given and an sd is
// non-zero, whoever is seated.  A guarded workgroup (pair index outside
// [0, K), a null or misaligned address) runs no tile and clears `in` of all
// its lanes: its games are not stepped and nothing of theirs is written, but
// it still advances the step slot (workgroup 0) and arrives for the ring and
// the call number.  Equal, bit for bit, to sk_actor_forward_f32 (32-row
// tiles) of every seated actor on the [2N] rows, each (seat, block) taking
// its actor's rows, followed by sk_env_step(_insert).
struct PoolArgs {
  const uint64_t* nets;  // [K][2]
  const int32_t* pairs;  // [P][2]
  int n_actors;
  int wgs_per_pair;      // block / 32
  int noisy_actor;       // -1: nobody
};
constexpr size_t kActPoolLds = kActorTileLds + 64 * sizeof(float2);
__global__ void __launch_bounds__(kFwdThreads, kPoolWaves) k_act_step_pool32(PoolArgs pl, float* __restrict__ act_out,
                                                                             float sd, float action_sd, uint64_t seed,
                                                                             uint64_t* __restrict__ call_ctr,
                                                                             sk::StepArgs a, sk::Cfg c) {
  extern __shared__ __attribute__((aligned(16))) float smem_sl[];
  char* smem = (char*)smem_sl;
  float2* sAct = (float2*)(smem + kActorTileLds);
  const int lane = threadIdx.x & 63;
  const bool w0 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) == 0;
  const int64_t g0 = (int64_t)blockIdx.x * 32;
  sk_counters* slot = a.ctr ? a.ctr + (size_t)blockIdx.x * SK_CTR_STRIDE : nullptr;
  const int p = (int)blockIdx.x / pl.wgs_per_pair;
  const int i1 = pl.pairs[2 * p], i2 = pl.pairs[2 * p + 1];
  uint64_t f1 = 0, k1 = 0, f2 = 0, k2 = 0;
  if ((unsigned)i1 < (unsigned)pl.n_actors && (unsigned)i2 < (unsigned)pl.n_actors) {
    f1 = pl.nets[2 * i1];
    k1 = pl.nets[2 * i1 + 1];
    f2 = pl.nets[2 * i2];
    k2 = pl.nets[2 * i2 + 1];
  }
  const bool ok = f1 && k1 && f2 && k2 && !((f1 | f2) & 3) && !((k1 | k2) & 15);
  sk::StepLane L;
  if (w0) {
    L = sk::split_load(a, 2 * g0 + lane, slot);
    if (!ok) L.in = false;
  }
  const bool draws = (sd != 0.f || action_sd != 0.f) && call_ctr;
  const uint64_t call = draws ? call_ctr[0] + 1 : 0;
  if (ok) {
#pragma unroll 1
    for (int seat = 0; seat < 2; ++seat) {
      const float* af = (const float*)(seat ? f2 : f1);
      const char* ap = (const char*)(seat ? k2 : k1);
      const bool noisy = (seat ? i2 : i1) == pl.noisy_actor;
      RowsSeatStore R;
      R.base = seat ? a.n : 0;
      R.g0 = g0;
      R.n = a.n;
      if (noisy && sd != 0.f)
        actor_tile32<true>(net_of(af, kALd, 2), ap, a.acting_obs, act_out, R, sd, action_sd, seed, call,
                           actor_lds(smem), sAct + 32 * seat);
      else
        actor_tile32<false>(net_of(af, kALd, 2), ap, a.acting_obs, act_out, R, 0.f, noisy ? action_sd : 0.f, seed,
                            call, actor_lds(smem), sAct + 32 * seat);
    }
  }
  __syncthreads();
  if (w0) sk::split_finish(a, c, L, ok ? sAct[(lane & 1) * 32 + (lane >> 1)] : make_float2(0.f, 0.f), slot);
  if (draws) {
    __syncthreads();
    advance_call32(call_ctr, call, gridDim.x);
  }
}
// The pool tick with scripted actors among its seats
// (sk_env_act_step_pool_bots): k_act_step_pool32 line for line (a kernel of
// its own, so that the net-only tick keeps its code), where a row of nets
// that bot_kind reads as a kind is a scripted actor.  Its seat runs no tile:
// after the seat loop wave 0's lanes of that seat compute the policy on what
// split_load loaded (sk::bot_lane, at the launch's step value) and store it
// to sAct and to `act_out`, as the tile would have.  A scripted actor draws
// no noise even when it is `noisy_actor`; the call number advances as above.
__global__ void __launch_bounds__(kFwdThreads, kPoolWaves) k_act_step_pool32_bots(
    PoolArgs pl, float* __restrict__ act_out, float sd, float action_sd, uint64_t seed,
    uint64_t* __restrict__ call_ctr, sk::StepArgs a, sk::Cfg c) {
  extern __shared__ __attribute__((aligned(16))) float smem_sl[];
  char* smem = (char*)smem_sl;
  float2* sAct = (float2*)(smem + kActorTileLds);
  const int lane = threadIdx.x & 63;
  const bool w0 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) == 0;
  const int64_t g0 = (int64_t)blockIdx.x * 32;
  sk_counters* slot = a.ctr ? a.ctr + (size_t)blockIdx.x * SK_CTR_STRIDE : nullptr;
  const int p = (int)blockIdx.x / pl.wgs_per_pair;
  const int i1 = pl.pairs[2 * p], i2 = pl.pairs[2 * p + 1];
  uint64_t f1 = 0, k1 = 0, f2 = 0, k2 = 0;
  if ((unsigned)i1 < (unsigned)pl.n_actors && (unsigned)i2 < (unsigned)pl.n_actors) {
    f1 = pl.nets[2 * i1];
    k1 = pl.nets[2 * i1 + 1];
    f2 = pl.nets[2 * i2];
    k2 = pl.nets[2 * i2 + 1];
  }
  const int b1 = bot_kind(f1, k1), b2 = bot_kind(f2, k2);
  const bool ok = (b1 || net_ok(f1, k1)) && (b2 || net_ok(f2, k2));
  sk::StepLane L;
  if (w0) {
    L = sk::split_load(a, 2 * g0 + lane, slot);
    if (!ok) L.in = false;
  }
  const bool draws = (sd != 0.f || action_sd != 0.f) && call_ctr;
  const uint64_t call = draws ? call_ctr[0] + 1 : 0;
  if (ok) {
#pragma unroll 1
    for (int seat = 0; seat < 2; ++seat) {
      if (seat ? b2 : b1) continue;  // workgroup-uniform
      const float* af = (const float*)(seat ? f2 : f1);
      const char* ap = (const char*)(seat ? k2 : k1);
      const bool noisy = (seat ? i2 : i1) == pl.noisy_actor;
      RowsSeatStore R;
      R.base = seat ? a.n : 0;
      R.g0 = g0;
      R.n = a.n;
      if (noisy && sd != 0.f)
        actor_tile32<true>(net_of(af, kALd, 2), ap, a.acting_obs, act_out, R, sd, action_sd, seed, call,
                           actor_lds(smem), sAct + 32 * seat);
      else
        actor_tile32<false>(net_of(af, kALd, 2), ap, a.acting_obs, act_out, R, 0.f, noisy ? action_sd : 0.f, seed,
                            call, actor_lds(smem), sAct + 32 * seat);
    }
    if (w0 && (b1 | b2)) {
      const int kind = (lane & 1) ? b2 : b1;
      const float2 b = sk::bot_lane(kind, lane & 1, L.pp, L.rot, c, a.seed, (uint64_t)(a.env_offset + L.ic), L.step);
      if (kind) {
        sAct[(lane & 1) * 32 + (lane >> 1)] = b;
        if (L.in) *(float2*)(act_out + ((int64_t)(lane & 1) * a.n + L.i) * 2) = b;
      }
    }
  }
  __syncthreads();
  if (w0) sk::split_finish(a, c, L, ok ? sAct[(lane & 1) * 32 + (lane >> 1)] : make_float2(0.f, 0.f), slot);
  if (draws) {
    __syncthreads();
    advance_call32(call_ctr, call, gridDim.x);
  }
}

// ---------------------------------------------------------------- actor forward, 16-row tiles
// The same forward for small row counts: a 32-row tile is a serial chain of
// load latencies around 3.4 us of MFMA per workgroup (9.4 us at 256 rows);
// 16-row tiles on v_mfma_f32_16x16x4_f32 halve the per-workgroup MFMA chain
// (6.5 us at 256 rows).  Above ~4,096 rows the 32-row tiles win: the chip's
// fp32 MFMA time dominates and two 16-row workgroups per CU contend.  Every weight
// fragment a wave needs before layer 2 is issued ahead of the staging
// barrier.  Wave w: layer-1 n-tiles w + 4q (16 units each), layer-2 n-tiles w
// and w + 4; layer 3 from DPP row sums of the layer-2 tiles.  The noise draws
// are keyed exactly as k_actor_fwd32's: normals4 per (first row of a 4-row
// group, unit), z[r] for row + r.
// The 16-row tile on the LDS at S / H1 / MP (kActorTile16Lds bytes) for the
// row map R (local row i -> global row; noise keyed by the global first row of
// each aligned 4-row group, so with N % 4 == 0 the players' map draws what
// the contiguous map draws).  k_actor_fwd16 (contiguous rows) runs it.
constexpr size_t kActorTile16Lds = (size_t)(kR * kLdS16 + kR * kLdH1) * 4 + 4 * kR * sizeof(f4);
template <bool NOISE, typename MAP>
__device__ __forceinline__ void actor_tile16(const Net& A, const float* __restrict__ X, float* __restrict__ out,
                                             const MAP& R, float sd, float action_sd, uint64_t seed, uint64_t call,
                                             float* S, float* H1, f4 (*MP)[kR], float2* act_lds) {
  const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, g = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  // ---- every load ahead of the barrier: states, layer-1 fragments and biases, the
  // first layer-2 fragments (g16_xwT256's prefetch), W3 / b2 of the wave's units
  const int si = tid >> 4, sk = tid & 15;
  const float sv = sk < kIn && R.valid(si) ? X[R(si) * kIn + sk] : 0.f;
  f4 w1v[4];
  float b1v[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    w1v[q] = w1_frag(A.W1, 16 * (w + 4 * q), lane);
    b1v[q] = A.b1[16 * (w + 4 * q) + i];
  }
  float b2v[2], w30[2], w31[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int u = 16 * (w + 4 * t) + i;
    b2v[t] = A.b2[u];
    w30[t] = A.W3[u];
    w31[t] = A.W3[kH2 + u];
  }
  S[si * kLdS16 + sk] = sv;
  lds_sync32();
  // ---- layer 1
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int u = 16 * (w + 4 * q) + i;
    const f4 x = *(const f4*)(S + i * kLdS16 + 4 * g);
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    const f32x4 m = m16x4(x, w1v[q], z4);
    const float b = b1v[q];
    if (NOISE) {
      const f32x4 var = m16x4(x * x, w1v[q] * w1v[q], z4);
      float y[4];
      noisy4(seed, call, (uint32_t)R(4 * g), (uint32_t)u, skmlp::noise_k2(sd), b, m, var, 0, y);
#pragma unroll
      for (int r = 0; r < 4; ++r) H1[(4 * g + r) * kLdH1 + u] = fmaxf(y[r], 0.f);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) H1[(4 * g + r) * kLdH1 + u] = fmaxf(m[r] + b, 0.f);
    }
  }
  lds_sync32();
  // ---- layer 2 (n-tiles w, w + 4) and the layer-3 partials of the wave's units
  // per row 4g + r: the layer-3 dot products (and their variances) over this lane's two units
  float pm0[4] = {0.f, 0.f, 0.f, 0.f}, pm1[4] = {0.f, 0.f, 0.f, 0.f}, pv0[4] = {0.f, 0.f, 0.f, 0.f},
        pv1[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int nt = w + 4 * t, u = 16 * nt + i;
    f32x4 m, var;
    if (NOISE) {
      g16_xwT256_mv(m, var, H1, A.W2, 16 * nt, lane);
    } else {
      m = g16_xwT256(H1, kLdH1, A.W2, kALd, 16 * nt, lane);
    }
    float yn[4];
    if (NOISE) noisy4(seed, call, (uint32_t)R(4 * g), (uint32_t)(kH1 + u), skmlp::noise_k2(sd), b2v[t], m, var, 0, yn);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float y = NOISE ? yn[r] : m[r] + b2v[t];
      const float h = fmaxf(y, 0.f);
      pm0[r] += h * w30[t];
      pm1[r] += h * w31[t];
      if (NOISE) {
        pv0[r] += h * h * w30[t] * w30[t];
        pv1[r] += h * h * w31[t] * w31[t];
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const f4 v = {rowsum16(pm0[r]), rowsum16(pm1[r]), NOISE ? rowsum16(pv0[r]) : 0.f, NOISE ? rowsum16(pv1[r]) : 0.f};
    if (i == 15) MP[w][4 * g + r] = v;
  }
  lds_sync32();
  // ---- layer 3, tanh, action noise: one thread per row
  if (tid < kR && R.valid(tid)) {
    const int64_t row = R(tid);
    const f4 v = (MP[0][tid] + MP[1][tid]) + (MP[2][tid] + MP[3][tid]);
    const float b30 = A.b3[0], b31 = A.b3[1];
    float y0 = v.x + b30, y1 = v.y + b31;
    if (NOISE) {
      float z[4];
      normals4(seed, call, (uint32_t)row, (uint32_t)(kH1 + kH2), z);
      y0 += sd * __builtin_amdgcn_sqrtf(v.z + b30 * b30) * z[0];
      y1 += sd * __builtin_amdgcn_sqrtf(v.w + b31 * b31) * z[1];
    }
    float o0 = tanhf(y0), o1 = tanhf(y1);
    if (action_sd != 0.f) {
      float z[4];
      normals4(seed, call, (uint32_t)row, (uint32_t)(kH1 + kH2 + 1), z);
      o0 += action_sd * z[0];
      o1 += action_sd * z[1];
    }
    *(float2*)(out + row * 2) = make_float2(o0, o1);
    if (act_lds) act_lds[tid] = make_float2(o0, o1);
  }
}

template <bool NOISE>
__global__ void __launch_bounds__(kFwdThreads) k_actor_fwd16(const float* __restrict__ aflat,
                                                             const float* __restrict__ X, float* __restrict__ out,
                                                             int64_t rows, float sd, float action_sd, uint64_t seed,
                                                             uint64_t* __restrict__ call_ctr) {
  __shared__ __attribute__((aligned(16))) float S[kR * kLdS16];
  __shared__ __attribute__((aligned(16))) float H1[kR * kLdH1];
  __shared__ __attribute__((aligned(16))) f4 MP[4][kR];  // per wave and row: {m0, m1, v0, v1} of layer 3
  const Net A = net_of(aflat, kALd, 2);
  const bool draws = (NOISE || action_sd != 0.f) && call_ctr;
  const uint64_t call = draws ? call_ctr[0] + 1 : 0;
  actor_tile16<NOISE>(A, X, out, RowsContig{(int64_t)blockIdx.x * kR, rows}, sd, action_sd, seed, call, S, H1, MP,
                      nullptr);
  if (draws) {
    __syncthreads();
    advance_call32(call_ctr, call, gridDim.x);
  }
}

// the split pack (sk_split.hpp) from the actor's flat fp32 parameters: one
// thread per plane element (the W1 padding k = 12..15 written as zero)
__global__ void k_split_pack32(const float* __restrict__ aflat, char* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  short* b;
  int idx, plane;
  float v;
  if (t < sksplit::kW1Plane) {
    idx = t;
    const int j = t & 7, lane = (t >> 3) & 63, nt = t >> 9;
    const int n = 32 * nt + (lane & 31), k = 8 * (lane >> 5) + j;
    v = k < kIn ? aflat[kPW1 + n * kIn + k] : 0.f;
    b = (short*)(out + sksplit::kOffW1);
    plane = sksplit::kW1Plane;
  } else if (t < sksplit::kW1Plane + sksplit::kW2Plane) {
    idx = t - sksplit::kW1Plane;
    const int j = idx & 7, lane = (idx >> 3) & 63, kk = (idx >> 9) & 15, nt = idx >> 13;
    const int o = 32 * nt + (lane & 31), i = 16 * kk + 8 * (lane >> 5) + j;
    v = aflat[kPW2 + o * kALd + i];
    b = (short*)(out + sksplit::kOffW2);
    plane = sksplit::kW2Plane;
  } else {
    return;
  }
  short hi, mid, lo, sq;
  sksplit::split4(v, hi, mid, lo, sq);
  b[idx] = hi;
  b[plane + idx] = mid;
  b[2 * plane + idx] = lo;
  b[3 * plane + idx] = sq;
}

// ---------------------------------------------------------------- host launchers
// 16-row actor forward up to 4,096 rows (at most half the CUs busy with 32-row
// tiles; profiles/r03u_actor_fwd.jsonl: 2,048 rows 9.6 -> 6.6 us, but 8,192
// rows 10.4 -> 10.9 us); SK_FWD16=0 / 1 forces the 32- / 16-row kernel
bool fwd16_rows(int64_t rows) {
  const char* e = getenv("SK_FWD16");
  const int v = e && *e ? atoi(e) : -1;
  return v == 1 || (v != 0 && rows <= 4096);
}

}  // namespace

// the self-play tick launch (sk_env_act_step, csrc/sk_engine.hip): a.n % 4 == 0
int sk_launch_act_step32(const float* aflat, const void* apack, float* act_out, float sd, float action_sd,
                         uint64_t seed, uint64_t* call_ctr, const sk::StepArgs& a, const sk::Cfg& c, hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    set_lds32(k_act_step32<true>, kActStepLds);
    set_lds32(k_act_step32<false>, kActStepLds);
    attr = true;
  }
  if (!apack || (((uintptr_t)apack) & 15)) return SK_EINVAL;  // the 32-row tile reads the split pack
  const unsigned G = (unsigned)((a.n + 15) / 16);
  const char* pk = (const char*)apack;
  if (sd != 0.f)
    k_act_step32<true><<<G, kFwdThreads, kActStepLds, st>>>(aflat, pk, act_out, sd, action_sd, seed, call_ctr, a, c);
  else
    k_act_step32<false><<<G, kFwdThreads, kActStepLds, st>>>(aflat, pk, act_out, 0.f, action_sd, seed, call_ctr, a,
                                                             c);
  return hipGetLastError() == hipSuccess ? SK_OK : SK_EHIP;
}

// the reference rule's episode collection (sk_env_act_episode, csrc/sk_engine.hip): a.n % 4 == 0
int sk_launch_act_episode32(const float* aflat, const void* apack, float sd, float action_sd, uint64_t seed,
                            uint64_t* call_ctr, const sk::StepArgs& a, const sk::Cfg& c, float* states,
                            float* actions, float* rewards, int32_t* lengths, int n_ticks, hipStream_t st) {
  constexpr size_t lds = kActStepLds + 16;
  static bool attr = false;
  if (!attr) {
    set_lds32(k_act_episode32<true>, lds);
    set_lds32(k_act_episode32<false>, lds);
    attr = true;
  }
  if (!apack || (((uintptr_t)apack) & 15)) return SK_EINVAL;
  const unsigned G = (unsigned)((a.n + 15) / 16);
  const EpisodeArgs ep{states, actions, rewards, lengths, n_ticks};
  const char* pk = (const char*)apack;
  if (sd != 0.f)
    k_act_episode32<true><<<G, kFwdThreads, lds, st>>>(aflat, pk, sd, action_sd, seed, call_ctr, a, c, ep);
  else
    k_act_episode32<false><<<G, kFwdThreads, lds, st>>>(aflat, pk, 0.f, action_sd, seed, call_ctr, a, c, ep);
  if (hipGetLastError() != hipSuccess) return SK_EHIP;
  const bool draws = (sd != 0.f || action_sd != 0.f) && call_ctr;
  k_episode_finish<<<1, 256, 0, st>>>(lengths, a.n, a.step, draws ? call_ctr : nullptr);
  return hipGetLastError() == hipSuccess ? SK_OK : SK_EHIP;
}

// The match family's launchers.  The entry points (csrc/sk_engine.hip) have checked every argument, a record
// against its launch included (rows, slabs, per_block, slab0 + n_ticks and every pointer); what a kernel's
// addressing rests on is checked here again.
// a seating: nets / pairs are device tables, a.n = n_pairs * block, block % 32 == 0
static bool seating_ok(const uint64_t* nets, int n_actors, const int32_t* pairs, int block, const sk::StepArgs& a) {
  return nets && pairs && n_actors >= 1 && block > 0 && block % 32 == 0 && a.n % block == 0;
}
// a record (or none) of a launch of `blocks` blocks of `block` games
static bool rec_ok(const sk_match_record* r, int64_t blocks, int64_t block) {
  return !r || (r->per_block >= 1 && r->per_block <= block && r->rows == blocks * r->per_block);
}
static RecArgs rec_args(const sk_match_record& r, int wgs_per_block) {
  return RecArgs{(int2*)r.states.pos,    (double*)r.states.rot,  (int2*)r.states.qpos, (double*)r.states.qrot,
                 (int2*)r.states.qcdage, (int2*)r.states.misc,   r.actions,            r.rewards,
                 (int64_t)r.rows,        r.per_block,            r.slab0,              wgs_per_block};
}
// behind a match kernel's launch: the step counter advances by max(lengths)
static int match_finish(const sk::StepArgs& a, int32_t* lengths, hipStream_t st) {
  if (hipGetLastError() != hipSuccess) return SK_EHIP;
  k_episode_finish<<<1, 256, 0, st>>>(lengths, a.n, a.step, nullptr);
  return hipGetLastError() == hipSuccess ? SK_OK : SK_EHIP;
}

// two actors' matches in one launch (sk_env_act_match / _rec): any a.n >= 1; rec: the record to keep, or NULL
int sk_launch_act_match32(const float* aflat1, const void* apack1, const float* aflat2, const void* apack2,
                          const sk::StepArgs& a, const sk::Cfg& c, float* obs2, float* returns, int32_t* lengths,
                          int32_t* last_half, int n_ticks, const sk_match_record* rec, hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    set_lds32(k_act_match32, kActMatchLds);
    set_lds32(k_act_match32_rec, kActMatchLds);
    attr = true;
  }
  if (!apack1 || !apack2 || ((((uintptr_t)apack1) | ((uintptr_t)apack2)) & 15)) return SK_EINVAL;
  if (!rec_ok(rec, 1, a.n)) return SK_EINVAL;
  const unsigned G = (unsigned)((a.n + 31) / 32);
  const char *pk1 = (const char*)apack1, *pk2 = (const char*)apack2;
  const MatchArgs mt{obs2, returns, lengths, last_half, n_ticks};
  if (rec)
    k_act_match32_rec<<<G, kFwdThreads, kActMatchLds, st>>>(aflat1, pk1, aflat2, pk2, a, c, mt, rec_args(*rec, 0));
  else
    k_act_match32<<<G, kFwdThreads, kActMatchLds, st>>>(aflat1, pk1, aflat2, pk2, a, c, mt);
  return match_finish(a, lengths, st);
}

// every pairing of a league in one launch (sk_env_act_league / _rec): a seating, a record or NULL
int sk_launch_act_league32(const uint64_t* nets, int n_actors, const int32_t* pairs, int block, const sk::StepArgs& a,
                           const sk::Cfg& c, float* obs2, float* returns, int32_t* lengths, int32_t* last_half,
                           int n_ticks, const sk_match_record* rec, hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    set_lds32(k_act_league32, kActMatchLds);
    set_lds32(k_act_league32_rec, kActMatchLds);
    attr = true;
  }
  if (!seating_ok(nets, n_actors, pairs, block, a) || !rec_ok(rec, a.n / block, block)) return SK_EINVAL;
  const unsigned G = (unsigned)(a.n / 32);
  const MatchArgs mt{obs2, returns, lengths, last_half, n_ticks};
  const LeagueArgs lg{nets, pairs, n_actors, block / 32};
  if (rec)
    k_act_league32_rec<<<G, kFwdThreads, kActMatchLds, st>>>(lg, a, c, mt, rec_args(*rec, block / 32));
  else
    k_act_league32<<<G, kFwdThreads, kActMatchLds, st>>>(lg, a, c, mt);
  return match_finish(a, lengths, st);
}

// the opponent-pool training tick (sk_env_act_step_pool): a seating
int sk_launch_act_step_pool32(const uint64_t* nets, int n_actors, const int32_t* pairs, int block, int noisy_actor,
                              float* act_out, float sd, float action_sd, uint64_t seed, uint64_t* call_ctr,
                              const sk::StepArgs& a, const sk::Cfg& c, hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    set_lds32(k_act_step_pool32, kActPoolLds);
    attr = true;
  }
  if (!seating_ok(nets, n_actors, pairs, block, a) || !act_out) return SK_EINVAL;
  if (noisy_actor < -1 || noisy_actor >= n_actors) return SK_EINVAL;
  const unsigned G = (unsigned)(a.n / 32);
  const PoolArgs pl{nets, pairs, n_actors, block / 32, noisy_actor};
  k_act_step_pool32<<<G, kFwdThreads, kActPoolLds, st>>>(pl, act_out, sd, action_sd, seed, call_ctr, a, c);
  return hipGetLastError() == hipSuccess ? SK_OK : SK_EHIP;
}

// the same two launches where rows of nets may name scripted actors (sk_env_act_league_bots / _bots_rec,
// sk_env_act_step_pool_bots): the _bots kernels, every check the net-only launchers make
int sk_launch_act_league32_bots(const uint64_t* nets, int n_actors, const int32_t* pairs, int block,
                                const sk::StepArgs& a, const sk::Cfg& c, float* obs2, float* returns, int32_t* lengths,
                                int32_t* last_half, int n_ticks, const sk_match_record* rec, hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    set_lds32(k_act_league32_bots<false>, kActMatchLds);
    set_lds32(k_act_league32_bots<true>, kActMatchLds);
    attr = true;
  }
  if (!seating_ok(nets, n_actors, pairs, block, a) || !rec_ok(rec, a.n / block, block)) return SK_EINVAL;
  const unsigned G = (unsigned)(a.n / 32);
  const MatchArgs mt{obs2, returns, lengths, last_half, n_ticks};
  const LeagueArgs lg{nets, pairs, n_actors, block / 32};
  if (rec)
    k_act_league32_bots<true><<<G, kFwdThreads, kActMatchLds, st>>>(lg, a, c, mt, rec_args(*rec, block / 32));
  else
    k_act_league32_bots<false><<<G, kFwdThreads, kActMatchLds, st>>>(lg, a, c, mt, RecArgs{});
  return match_finish(a, lengths, st);
}

// the league with its statistics (sk_env_act_league_stats): the _bots launcher's checks; stats int32
// [SK_N_STATS + 2][2][a.n], the tick limit within skstat::fits
int sk_launch_act_league32_stats(const uint64_t* nets, int n_actors, const int32_t* pairs, int block,
                                 const sk::StepArgs& a, const sk::Cfg& c, float* obs2, float* returns, int32_t* lengths,
                                 int32_t* last_half, int n_ticks, int32_t* stats, const sk_match_record* rec,
                                 hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    set_lds32(k_act_league32_stats<false>, kActMatchLds);
    set_lds32(k_act_league32_stats<true>, kActMatchLds);
    attr = true;
  }
  if (!seating_ok(nets, n_actors, pairs, block, a) || !rec_ok(rec, a.n / block, block)) return SK_EINVAL;
  if (!stats || (((uintptr_t)stats) & 3) || !skstat::fits(a.tick_limit, c.W, c.H)) return SK_EINVAL;
  const unsigned G = (unsigned)(a.n / 32);
  const MatchArgs mt{obs2, returns, lengths, last_half, n_ticks};
  const LeagueArgs lg{nets, pairs, n_actors, block / 32};
  if (rec)
    k_act_league32_stats<true><<<G, kFwdThreads, kActMatchLds, st>>>(lg, a, c, mt, rec_args(*rec, block / 32), stats);
  else
    k_act_league32_stats<false><<<G, kFwdThreads, kActMatchLds, st>>>(lg, a, c, mt, RecArgs{}, stats);
  return match_finish(a, lengths, st);
}

int sk_launch_act_step_pool32_bots(const uint64_t* nets, int n_actors, const int32_t* pairs, int block,
                                   int noisy_actor, float* act_out, float sd, float action_sd, uint64_t seed,
                                   uint64_t* call_ctr, const sk::StepArgs& a, const sk::Cfg& c, hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    set_lds32(k_act_step_pool32_bots, kActPoolLds);
    attr = true;
  }
  if (!seating_ok(nets, n_actors, pairs, block, a) || !act_out) return SK_EINVAL;
  if (noisy_actor < -1 || noisy_actor >= n_actors) return SK_EINVAL;
  const unsigned G = (unsigned)(a.n / 32);
  const PoolArgs pl{nets, pairs, n_actors, block / 32, noisy_actor};
  k_act_step_pool32_bots<<<G, kFwdThreads, kActPoolLds, st>>>(pl, act_out, sd, action_sd, seed, call_ctr, a, c);
  return hipGetLastError() == hipSuccess ? SK_OK : SK_EHIP;
}

extern "C" {

int sk_actor_forward_f32(const float* actor_flat, const void* actor_pack, const float* obs, float* actions,
                         int64_t rows, float noise_sd, float action_sd, uint64_t seed, uint64_t* call_counter,
                         void* stream) {
  if (!actor_flat || !obs || !actions || rows <= 0) return SK_EINVAL;
  if ((((uintptr_t)actions) & 7)) return SK_EINVAL;
  if (fwd16_rows(rows)) {
    const unsigned G16 = (unsigned)((rows + kR - 1) / kR);
    if (noise_sd != 0.f)
      k_actor_fwd16<true><<<G16, kFwdThreads, 0, (hipStream_t)stream>>>(actor_flat, obs, actions, rows, noise_sd,
                                                                          action_sd, seed, call_counter);
    else
      k_actor_fwd16<false><<<G16, kFwdThreads, 0, (hipStream_t)stream>>>(actor_flat, obs, actions, rows, 0.f,
                                                                           action_sd, seed, call_counter);
    return hipGetLastError() == hipSuccess ? SK_OK : SK_EHIP;
  }
  if (!actor_pack || (((uintptr_t)actor_pack) & 15)) return SK_EINVAL;  // the 32-row tile reads the split pack
  static bool attr = false;
  if (!attr) {
    set_lds32(k_actor_fwd32<true>, kActorTileLds);
    set_lds32(k_actor_fwd32<false>, kActorTileLds);
    attr = true;
  }
  const unsigned G = (unsigned)((rows + 31) / 32);
  const char* pk = (const char*)actor_pack;
  if (noise_sd != 0.f)
    k_actor_fwd32<true><<<G, kFwdThreads, kActorTileLds, (hipStream_t)stream>>>(actor_flat, pk, obs, actions, rows,
                                                                                 noise_sd, action_sd, seed,
                                                                                 call_counter);
  else
    k_actor_fwd32<false><<<G, kFwdThreads, kActorTileLds, (hipStream_t)stream>>>(actor_flat, pk, obs, actions, rows,
                                                                                  0.f, action_sd, seed, call_counter);
  return hipGetLastError() == hipSuccess ? SK_OK : SK_EHIP;
}

size_t sk_actor_split_pack_bytes(void) { return sksplit::kBytes; }

int sk_actor_split_pack_f32(const float* actor_flat, void* actor_pack, void* stream) {
  if (!actor_flat || !actor_pack || (((uintptr_t)actor_pack) & 15)) return SK_EINVAL;
  const int n = sksplit::kW1Plane + sksplit::kW2Plane;  // one thread per plane-0 element
  k_split_pack32<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(actor_flat, (char*)actor_pack);
  return hipGetLastError() == hipSuccess ? SK_OK : SK_EHIP;
}

}  // extern "C"

#endif  // SK_ACT32_HPP
