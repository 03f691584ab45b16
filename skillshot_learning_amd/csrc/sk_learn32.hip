// sk_learn32.hip — the learner at the reference's precision, fp32 operands
// and fp32 accumulation, for the Keras fp32 nets of SkillshotLearner.py:70-121
// and their update (:386-443).  This file holds the gradient half and the C
// entry points; the acting half (the actor forward, the self-play tick, the
// episode, match, league, recording and pool-tick kernels and their launchers,
// one per kernel family: a recording twin is launched by its plain kernel's
// launcher, given a match record) is sk_act32.hpp,
// included below into this translation unit, and what both halves share
// (the nets' views, Philox, the MFMA fragments, the size constants) is
// sk_net32.hpp.
//
//   k_critic_grad32   critic train step: (bootstrap target from the target
//                     nets,) Dropout(0.2) forward, MSE, backward ->
//                     per-workgroup gradient partials
//   k_actor_grad32    actor step: actor forward, critic forward at inference,
//                     dQ/da, backward of -sum Q -> per-workgroup partials
//   k_grad_slice_fwd / k_grad_slice_bwd
//                     the same two steps for small minibatches, layer 2 split
//                     over 8 workgroups per row tile (launch_sliced)
//   k_bwd_act_step32  the sliced backward with the next acting tick
//                     (sk_act32.hpp's act_step32) beside it in one launch:
//                     the one place the two halves meet
// The partials are summed (and Adam applied) by k_adam_flat (sk_update.hip).
//
// No packing: the kernels read the weights straight from the nets' flat fp32
// parameter vectors in torch parameters() order (update_kernel.flatten_module)
// W1 [256][12], b1, W2 [128][ld2], b2, W3 [n_out][128], b3 (ld2 = 258 for the
// critic: the last two columns multiply the action).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <cstring>

#include "../../include/skillshot.h"
#include "sk_act32.hpp"
#include "sk_mlp.hpp"
#include "sk_net32.hpp"
#include "sk_partial.hpp"
#include "sk_step.hpp"

namespace {

// fp32 tails of a net staged in LDS (1024 floats, the bf16 grad-pack tail
// layout): b1 [256], b2 [128], critic action columns W2[u][256 + j] as [128][2],
// W3 [n_out][128], b3
constexpr int kT1 = 0, kT2 = 256, kTA = 384, kT3 = 640, kTB = 896;
// One load per element from an index chosen by selects: a load per branch
// put each element's candidate loads in one VGPR, and the write-after-write
// between them cost an s_waitcnt vmcnt(0) -- a full round trip of every load
// in flight -- per branch a wave took (profiles/r04ao_trace_slice_bwd.jsonl).
__device__ __forceinline__ float tail_src(gfp f, int ld2, int n_out, int e) {
  const int ea = e - kTA, e3 = e - kT3, eb = e - kTB;
  int idx = e < kT2 ? kPB1 + e : pB2(ld2) + e - kT2;
  // (a 24-bit product: the 32-bit one became a v_mad_u64_u32 whose unused
  // high addend half was a register with a load in flight)
  idx = e < kTA ? idx : kPW2 + (int)__umul24((unsigned)ea >> 1, (unsigned)ld2) + kH1 + (ea & 1);
  idx = e < kT3 ? idx : pW3(ld2) + e3;
  idx = e < kTB ? idx : pB3(ld2, n_out) + eb;
  const bool ok = e < kTA || (e < kT3 ? ld2 != kH1 : e < kTB ? e3 < n_out * kH2 : eb < n_out);
  const float v = f[ok ? idx : 0];
  return ok ? v : 0.f;
}

struct G32 {
  float *S, *S2, *ST, *H1, *H1a, *H1c, *H1T, *DZ2, *DZ2T, *DZ1T, *TL, *A, *R, *D, *Y, *QP, *MP, *YP, *DP, *RED;
};
constexpr int kG32Floats = 3 * kR * kLdS16 + 3 * kR * kLdH1 + kH1 * kLdT16 + kR * kLdH2 + kH2 * kLdT16 +
                           kH1 * kLdT16 + 3 * 1024 + 32 + 16 + 16 + 16 + 8 * 16 + 8 * 32 + 8 * 16 + 8 * 32 + 4;
constexpr size_t kLdsGrad32 = (size_t)kG32Floats * 4;
static_assert(kLdsGrad32 <= 160 * 1024, "LDS budget of one CU");
__device__ __forceinline__ G32 carve32(float* p) {
  G32 L;
  L.S = p;    p += kR * kLdS16;
  L.S2 = p;   p += kR * kLdS16;
  L.ST = p;   p += kR * kLdS16;
  L.H1 = p;   p += kR * kLdH1;
  L.H1a = p;  p += kR * kLdH1;
  L.H1c = p;  p += kR * kLdH1;
  L.H1T = p;  p += kH1 * kLdT16;
  L.DZ2 = p;  p += kR * kLdH2;
  L.DZ2T = p; p += kH2 * kLdT16;
  L.DZ1T = p; p += kH1 * kLdT16;
  L.TL = p;   p += 3 * 1024;
  L.A = p;    p += 32;
  L.R = p;    p += 16;
  L.D = p;    p += 16;
  L.Y = p;    p += 16;
  L.QP = p;   p += 8 * 16;  // per-wave partial row sums: [wave][row]
  L.MP = p;   p += 8 * 32;  //                             [wave][row][2]
  L.YP = p;   p += 8 * 16;
  L.DP = p;   p += 8 * 32;
  L.RED = p;
  return L;
}
// Dropout keep bits of n-tiles w and w + 8 (16 units each): bit 4j + r is
// row 4g + r of the sub-tile, unit 16 (w + 8j) + i (rng.dropout_keep: the mask
// of global row key + row, Philox word row % 4 of counter (row / 4, unit))
__device__ __forceinline__ uint32_t dropout_bits16(uint64_t seed, uint64_t call, int64_t key, int w, int lane) {
  const int i = lane & 15, g = lane >> 4;
  uint32_t bits = 0;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const uint4 u = philox(make_uint4((uint32_t)((key + 4 * g) >> 2), (uint32_t)(16 * (w + 8 * j) + i), (uint32_t)call,
                                      (uint32_t)(call >> 32)),
                           (uint32_t)seed, (uint32_t)(seed >> 32));
    bits |= ((uint32_t)(u.x >= 858993460u) | ((uint32_t)(u.y >= 858993460u) << 1) |
             ((uint32_t)(u.z >= 858993460u) << 2) | ((uint32_t)(u.w >= 858993460u) << 3)) << (4 * j);
  }
  return bits;
}
// layer-1 epilogue of n-tile nt: relu(acc + b1) (x Dropout keep bits) ->
// H [row][unit] and, if HT, HT [unit][rows] (one 16-byte write)
__device__ __forceinline__ void l1_out(f32x4 acc, const float* tl, int nt, int lane, float* H, float* HT, bool drop,
                                       uint32_t bits4) {
  const int i = lane & 15, g = lane >> 4, n = 16 * nt + i;
  const float b = tl[kT1 + n];
  f4 z;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float v = fmaxf(acc[r] + b, 0.f);
    if (drop) v = (bits4 >> r) & 1u ? v * 1.25f : 0.f;
    z[r] = v;
    H[(4 * g + r) * kLdH1 + n] = v;
  }
  if (HT) *(f4*)(HT + n * kLdT16 + 4 * g) = z;
}

// ---------------------------------------------------------------- critic step
// Critic.forward in training mode + MSE backward (critic.fit,
// SkillshotLearner.py:434; DDPG.critic_step): dL/dq = grad_scale (q - y),
// grad_scale = 2 / global batch; Dropout keep-mask of global row key_row0 +
// row (rng.dropout_keep), keep -> x 1.25.  BOOT: y = r + gamma (1 - done)
// Q'(s', mu'(s')) from the target nets, in the same phases (wave w: layer-2
// unit tile w, layer-1 / dz1 tiles w and w + 8):
//   0  stage s, a (s', r, done), the nets' tails; Dropout bits meanwhile
//   1  layer 1 of the critic (Dropout), the target actor, the target critic
//   2  layer 2 of the critic and of the target actor (chains interleaved);
//      per-wave partial row sums of q and mu'
//   3  mu'(s') from the partials; the target critic's layer 2 -> Q' partials
//   4  y, dL/dq per row; dz2 of the wave's units
//   5  dW2 (16 tiles per wave), dz1;  6  dW1
template <bool BOOT>
__global__ void __launch_bounds__(kThreads) k_critic_grad32(
    const float* __restrict__ cflat, const float* __restrict__ Sg, const float* __restrict__ Ag,
    const float* __restrict__ Yg, int64_t B, int64_t key_row0, int sub_per_wg, float grad_scale, uint64_t seed,
    const int64_t* __restrict__ call_ctr, float* __restrict__ partial, float* step_ctr, int n_steps,
    float* __restrict__ loss_out, uint8_t* __restrict__ mask_out, const float* __restrict__ S2g,
    const float* __restrict__ Rg, const float* __restrict__ Dg, float gamma, const float* __restrict__ taflat,
    const float* __restrict__ tcflat) {
  extern __shared__ __attribute__((aligned(16))) float smem32[];
  const G32 L = carve32(smem32);
  TP32(0);
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t call = (uint64_t)*call_ctr;
  if (blockIdx.x == 0 && threadIdx.x < n_steps) step_ctr[threadIdx.x] += 1.0f;  // Adam's step (read by k_adam_flat)
  const float* TLc = L.TL;
  const float* TLa = L.TL + 1024;
  const float* TLt = L.TL + 2048;
  f32x4 gW2[16], gW1[2];
#pragma unroll
  for (int t = 0; t < 16; ++t) gW2[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  gW1[0] = gW1[1] = f32x4{0.f, 0.f, 0.f, 0.f};
  // per-lane partial sums: b1 of units 16(w + 8j) + i, b2 / W2 action
  // columns / W3 of unit 16w + i (over the lane's rows), db3 and the loss
  float gb1[2] = {0.f, 0.f}, gb2 = 0.f, gwa0 = 0.f, gwa1 = 0.f, gw3 = 0.f, gb3 = 0.f, lsum = 0.f;
  if (threadIdx.x < 4) L.RED[threadIdx.x] = 0.f;
  for (int sub = 0; sub < sub_per_wg; ++sub) {
    const int64_t row0 = ((int64_t)blockIdx.x * sub_per_wg + sub) * kR;
    if (row0 >= B) break;  // uniform across the workgroup
    const int tid = launder_lane(threadIdx.x), lane = tid & 63, i = lane & 15, g = lane >> 4;
    const int u = 16 * w + i;  // the lane's layer-2 unit
    const Net C = net_of(launder(cflat), kCLd, 1);
    // ---- phase 0: every global load, the Dropout bits while they fly, then LDS
    const int si = (tid & 255) >> 4, sk = tid & 15;
    const float* src = tid < 256 ? Sg : S2g;
    const bool want_s = tid < 256 || BOOT;
    const float sv = want_s && sk < kIn && row0 + si < B ? src[(row0 + si) * kIn + sk] : 0.f;
    const float av = tid < 32 && row0 + (tid >> 1) < B ? Ag[row0 * 2 + tid] : 0.f;
    const bool rok = tid < kR && row0 + tid < B;
    const float rv = rok ? (BOOT ? Rg[row0 + tid] : Yg[row0 + tid]) : 0.f;
    const float dv = BOOT && rok ? Dg[row0 + tid] : 0.f;
    float tv[6];
    if (sub == 0) {
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const int net = k >> 1, e = tid + kThreads * (k & 1);
        tv[k] = net == 0 ? tail_src(C.W1, kCLd, 1, e)
                         : (BOOT ? (net == 1 ? tail_src((gfp)launder(taflat), kALd, 2, e)
                                             : tail_src((gfp)launder(tcflat), kCLd, 1, e))
                                 : 0.f);
      }
    }
    uint32_t keep = dropout_bits16(seed, call, key_row0 + row0, w, lane);
    asm volatile("" : "+v"(keep));  // computed here, under the loads' latency
    if (mask_out) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (row0 + 4 * g + r < B) mask_out[(row0 + 4 * g + r) * kH1 + 16 * (w + 8 * j) + i] = (keep >> (4 * j + r)) & 1u;
    }
    if (tid < 256) {
      L.S[si * kLdS16 + sk] = sv;
      L.ST[sk * kLdT16 + si] = sv;  // feature rows 12..15 get zeros
    } else if (BOOT) {
      L.S2[si * kLdS16 + sk] = sv;
    }
    if (tid < 32) L.A[tid] = av;
    if (tid < kR) {
      if (BOOT) {
        L.R[tid] = rv;
        L.D[tid] = dv;
      } else {
        L.Y[tid] = rv;
      }
    }
    if (sub == 0) {
#pragma unroll
      for (int k = 0; k < 6; ++k)
        if (k < 2 || BOOT) L.TL[(k >> 1) * 1024 + tid + kThreads * (k & 1)] = tv[k];
    }
    lds_sync32();
    TP32(1);
    // ---- phase 1: layer 1, n-tiles w and w + 8, of the critic (Dropout), target actor, target critic
    const Net TA = net_of(launder(BOOT ? taflat : cflat), kALd, 2), TC = net_of(launder(BOOT ? tcflat : cflat), kCLd, 1);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int nt = w + 8 * j;
      l1_out(g16_l1(L.S, C.W1, 16 * nt, lane), TLc, nt, lane, L.H1, L.H1T, true, keep >> (4 * j));
      if (BOOT) {
        l1_out(g16_l1(L.S2, TA.W1, 16 * nt, lane), TLa, nt, lane, L.H1a, nullptr, false, 0);
        l1_out(g16_l1(L.S2, TC.W1, 16 * nt, lane), TLt, nt, lane, L.H1c, nullptr, false, 0);
      }
    }
    lds_sync32();
    TP32(2);
    // ---- phase 2: critic h2 (registers) and per-wave q partials; target actor mu' partials
    float h2[4];
    {
      f32x4 acc, acca;
      if (BOOT) g16_xwT256x2(acc, acca, L.H1, C.W2, kCLd, L.H1a, TA.W2, kALd, 16 * w, lane);
      else acc = g16_xwT256(L.H1, kLdH1, C.W2, kCLd, 16 * w, lane);
      const float b2 = TLc[kT2 + u], wa0 = TLc[kTA + 2 * u], wa1 = TLc[kTA + 2 * u + 1], w3 = TLc[kT3 + u];
      const f4 a01 = *(const f4*)(L.A + 8 * g), a23 = *(const f4*)(L.A + 8 * g + 4);  // a[4g + r][0..1]
      const float a0[4] = {a01.x, a01.z, a23.x, a23.z}, a1[4] = {a01.y, a01.w, a23.y, a23.w};
      f4 qp;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        h2[r] = fmaxf(acc[r] + b2 + a0[r] * wa0 + a1[r] * wa1, 0.f);
        qp[r] = rowsum16(h2[r] * w3);
      }
      if (i == 15) *(f4*)(L.QP + 16 * w + 4 * g) = qp;
      if (BOOT) {
        const float b2a = TLa[kT2 + u], w30 = TLa[kT3 + u], w31 = TLa[kT3 + kH2 + u];
        f4 m0, m1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float h = fmaxf(acca[r] + b2a, 0.f);
          m0[r] = rowsum16(h * w30);
          m1[r] = rowsum16(h * w31);
        }
        if (i == 15) {
          *(f4*)(L.MP + 32 * w + 8 * g) = f4{m0.x, m1.x, m0.y, m1.y};
          *(f4*)(L.MP + 32 * w + 8 * g + 4) = f4{m0.z, m1.z, m0.w, m1.w};
        }
      }
    }
    lds_sync32();
    TP32(3);
    // ---- phase 3 (BOOT): mu'(s') of the lane's rows, the target critic's layer 2 -> Q' partials
    if (BOOT) {
      f4 s01 = {0.f, 0.f, 0.f, 0.f}, s23 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int v = 0; v < 8; ++v) {
        s01 += *(const f4*)(L.MP + 32 * v + 8 * g);
        s23 += *(const f4*)(L.MP + 32 * v + 8 * g + 4);
      }
      const float ap0[4] = {tanhf(s01.x + TLa[kTB]), tanhf(s01.z + TLa[kTB]), tanhf(s23.x + TLa[kTB]),
                            tanhf(s23.z + TLa[kTB])};
      const float ap1[4] = {tanhf(s01.y + TLa[kTB + 1]), tanhf(s01.w + TLa[kTB + 1]), tanhf(s23.y + TLa[kTB + 1]),
                            tanhf(s23.w + TLa[kTB + 1])};
      const f32x4 acc = g16_xwT256(L.H1c, kLdH1, TC.W2, kCLd, 16 * w, lane);
      const float b2 = TLt[kT2 + u], wa0 = TLt[kTA + 2 * u], wa1 = TLt[kTA + 2 * u + 1], w3 = TLt[kT3 + u];
      f4 yp;
#pragma unroll
      for (int r = 0; r < 4; ++r) yp[r] = rowsum16(fmaxf(acc[r] + b2 + ap0[r] * wa0 + ap1[r] * wa1, 0.f) * w3);
      if (i == 15) *(f4*)(L.YP + 16 * w + 4 * g) = yp;
      lds_sync32();
    }
    TP32(4);
    // ---- phase 4: y and dL/dq of the lane's rows; dz2 = dL/dq W3 relu'(h2) of unit u
    {
      f4 q = {TLc[kTB], TLc[kTB], TLc[kTB], TLc[kTB]}, yq = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int v = 0; v < 8; ++v) {
        q += *(const f4*)(L.QP + 16 * v + 4 * g);
        if (BOOT) yq += *(const f4*)(L.YP + 16 * v + 4 * g);
      }
      const f4 rr = *(const f4*)((BOOT ? L.R : L.Y) + 4 * g);
      const f4 dd = BOOT ? *(const f4*)(L.D + 4 * g) : f4{0.f, 0.f, 0.f, 0.f};
      const float w3 = TLc[kT3 + u];
      const f4 a01 = *(const f4*)(L.A + 8 * g), a23 = *(const f4*)(L.A + 8 * g + 4);
      const float a0[4] = {a01.x, a01.z, a23.x, a23.z}, a1[4] = {a01.y, a01.w, a23.y, a23.w};
      f4 dz;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float y = BOOT ? rr[r] + gamma * (1.f - dd[r]) * (TLt[kTB] + yq[r]) : rr[r];
        const float e = row0 + 4 * g + r < B ? q[r] - y : 0.f;
        const float dq = grad_scale * e;
        if (w == 0 && i == 0) {
          gb3 += dq;
          lsum += e * e;
        }
        const float d = h2[r] > 0.f ? dq * w3 : 0.f;
        dz[r] = d;
        L.DZ2[(4 * g + r) * kLdH2 + u] = d;
        gb2 += d;
        gwa0 += d * a0[r];
        gwa1 += d * a1[r];
        gw3 += dq * h2[r];
      }
      *(f4*)(L.DZ2T + u * kLdT16 + 4 * g) = dz;
    }
    lds_sync32();
    TP32(5);
    // ---- phase 5: dW2 (unit tile w x 16 input tiles), dz1 of n-tiles w, w + 8
#pragma unroll
    for (int kt = 0; kt < 16; ++kt) gW2[kt] = g16_wgrad(gW2[kt], L.DZ2T, 16 * w, L.H1T, 16 * kt, lane);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = 16 * (w + 8 * j) + i;
      const f32x4 acc = g16_xw128(L.DZ2, kLdH2, C.W2, kCLd, 16 * (w + 8 * j), lane);
      f4 d;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        d[r] = L.H1[(4 * g + r) * kLdH1 + n] > 0.f ? acc[r] * 1.25f : 0.f;
        gb1[j] += d[r];
      }
      *(f4*)(L.DZ1T + n * kLdT16 + 4 * g) = d;
    }
    lds_sync32();
    TP32(6);
    // ---- phase 6: dW1 of unit tiles w, w + 8 (input columns 12..15 discarded)
#pragma unroll
    for (int j = 0; j < 2; ++j) gW1[j] = g16_wgrad(gW1[j], L.DZ1T, 16 * (w + 8 * j), L.ST, 0, lane);
    lds_sync32();  // the next sub-tile restages
    TP32(7);
  }
  // ---- this workgroup's partial gradient (sk_partial.hpp layout)
  float* P = partial + (int64_t)blockIdx.x * kCP;
  const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4, u = 16 * w + i;
#pragma unroll
  for (int kt = 0; kt < 16; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) P[skpart::critic_w2_main(16 * w + 4 * g + r, 16 * kt + i)] = gW2[kt][r];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (i < kIn) {
#pragma unroll
      for (int r = 0; r < 4; ++r) P[kPW1 + (16 * (w + 8 * j) + 4 * g + r) * kIn + i] = gW1[j][r];
    }
    float b = gb1[j] + __shfl_xor(gb1[j], 16, 64);
    b += __shfl_xor(b, 32, 64);
    if (g == 0) P[kPB1 + 16 * (w + 8 * j) + i] = b;
  }
  TP32(8);
  gb2 += __shfl_xor(gb2, 16, 64);
  gb2 += __shfl_xor(gb2, 32, 64);
  gwa0 += __shfl_xor(gwa0, 16, 64);
  gwa0 += __shfl_xor(gwa0, 32, 64);
  gwa1 += __shfl_xor(gwa1, 16, 64);
  gwa1 += __shfl_xor(gwa1, 32, 64);
  gw3 += __shfl_xor(gw3, 16, 64);
  gw3 += __shfl_xor(gw3, 32, 64);
  if (g == 0) {
    P[pB2(kCLd) + u] = gb2;
    P[skpart::critic_w2_action(u, 0)] = gwa0;
    P[skpart::critic_w2_action(u, 1)] = gwa1;
    P[pW3(kCLd) + u] = gw3;
  }
  if (w == 0 && i == 0) {  // wave 0, one lane per row group: db3 and loss partials
    atomicAdd(&L.RED[0], gb3);
    atomicAdd(&L.RED[1], lsum);
  }
  lds_sync32();
  if (threadIdx.x == 0) {
    P[pB3(kCLd, 1)] = L.RED[0];
    if (loss_out) atomicAdd(loss_out, L.RED[1]);
  }
  TP32(9);
}

// ---------------------------------------------------------------- actor step
// model_actor_fit_step (SkillshotLearner.py:386-417): gradient of
// -loss_scale * sum_b Q(s_b, mu(s_b)) w.r.t. the actor, critic at inference.
//   0  stage s, the nets' tails
//   1  layer 1 of the actor (-> H1, H1T) and of the critic (-> H1c)
//   2  the actor's layer 2 (-> h2 registers, mu partials) and the critic's
//      layer-2 MFMA (held; its action columns join in phase 3), interleaved
//   3  mu per row; critic z2 at (s, mu): dQ/da and Q partials
//   4  dL/dz3 = -loss_scale dQ/da (1 - a^2) per row; dz2 of unit 16w + i
//   5  dW2, dz1;  6  dW1
__global__ void __launch_bounds__(kThreads) k_actor_grad32(const float* __restrict__ aflat,
                                                           const float* __restrict__ cflat,
                                                           const float* __restrict__ Sg, int64_t B, int sub_per_wg,
                                                           float loss_scale, float* __restrict__ partial,
                                                           float* step_ctr, int n_steps, float* __restrict__ q_out) {
  extern __shared__ __attribute__((aligned(16))) float smem32[];
  const G32 L = carve32(smem32);
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (blockIdx.x == 0 && threadIdx.x < n_steps) step_ctr[threadIdx.x] += 1.0f;
  const float* TLa = L.TL;
  const float* TLc = L.TL + 1024;
  f32x4 gW2[16], gW1[2];
#pragma unroll
  for (int t = 0; t < 16; ++t) gW2[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  gW1[0] = gW1[1] = f32x4{0.f, 0.f, 0.f, 0.f};
  float gb1[2] = {0.f, 0.f}, gb2 = 0.f, gw30 = 0.f, gw31 = 0.f, gb30 = 0.f, gb31 = 0.f, qsum = 0.f;
  if (threadIdx.x < 4) L.RED[threadIdx.x] = 0.f;
  for (int sub = 0; sub < sub_per_wg; ++sub) {
    const int64_t row0 = ((int64_t)blockIdx.x * sub_per_wg + sub) * kR;
    if (row0 >= B) break;
    const int tid = launder_lane(threadIdx.x), lane = tid & 63, i = lane & 15, g = lane >> 4;
    const int u = 16 * w + i;
    const Net A = net_of(launder(aflat), kALd, 2), C = net_of(launder(cflat), kCLd, 1);
    // ---- phase 0
    const int si = tid >> 4, sk = tid & 15;
    const float sv = tid < 256 && sk < kIn && row0 + si < B ? Sg[(row0 + si) * kIn + sk] : 0.f;
    float tv[4];
    if (sub == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int e = tid + kThreads * (k & 1);
        tv[k] = k < 2 ? tail_src(A.W1, kALd, 2, e) : tail_src(C.W1, kCLd, 1, e);
      }
    }
    if (tid < 256) {
      L.S[si * kLdS16 + sk] = sv;
      L.ST[sk * kLdT16 + si] = sv;
    }
    if (sub == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) L.TL[(k >> 1) * 1024 + tid + kThreads * (k & 1)] = tv[k];
    }
    lds_sync32();
    // ---- phase 1
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int nt = w + 8 * j;
      l1_out(g16_l1(L.S, A.W1, 16 * nt, lane), TLa, nt, lane, L.H1, L.H1T, false, 0);
      l1_out(g16_l1(L.S, C.W1, 16 * nt, lane), TLc, nt, lane, L.H1c, nullptr, false, 0);
    }
    lds_sync32();
    // ---- phase 2
    float h2[4];
    f32x4 zc;
    {
      f32x4 acc;
      g16_xwT256x2(acc, zc, L.H1, A.W2, kALd, L.H1c, C.W2, kCLd, 16 * w, lane);
      const float b2 = TLa[kT2 + u], w30 = TLa[kT3 + u], w31 = TLa[kT3 + kH2 + u];
      f4 m0, m1;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        h2[r] = fmaxf(acc[r] + b2, 0.f);
        m0[r] = rowsum16(h2[r] * w30);
        m1[r] = rowsum16(h2[r] * w31);
      }
      if (i == 15) {
        *(f4*)(L.MP + 32 * w + 8 * g) = f4{m0.x, m1.x, m0.y, m1.y};
        *(f4*)(L.MP + 32 * w + 8 * g + 4) = f4{m0.z, m1.z, m0.w, m1.w};
      }
    }
    lds_sync32();
    // ---- phase 3: mu of the lane's rows; the critic at (s, mu)
    float a0[4], a1[4];
    {
      f4 s01 = {0.f, 0.f, 0.f, 0.f}, s23 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int v = 0; v < 8; ++v) {
        s01 += *(const f4*)(L.MP + 32 * v + 8 * g);
        s23 += *(const f4*)(L.MP + 32 * v + 8 * g + 4);
      }
      a0[0] = tanhf(s01.x + TLa[kTB]);
      a1[0] = tanhf(s01.y + TLa[kTB + 1]);
      a0[1] = tanhf(s01.z + TLa[kTB]);
      a1[1] = tanhf(s01.w + TLa[kTB + 1]);
      a0[2] = tanhf(s23.x + TLa[kTB]);
      a1[2] = tanhf(s23.y + TLa[kTB + 1]);
      a0[3] = tanhf(s23.z + TLa[kTB]);
      a1[3] = tanhf(s23.w + TLa[kTB + 1]);
      const float b2 = TLc[kT2 + u], wa0 = TLc[kTA + 2 * u], wa1 = TLc[kTA + 2 * u + 1], w3 = TLc[kT3 + u];
      f4 d0, d1, qp;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float z = zc[r] + b2 + a0[r] * wa0 + a1[r] * wa1;
        const float dqdz = (z > 0.f && row0 + 4 * g + r < B) ? w3 : 0.f;  // dQ/dz2 (rows beyond B: 0)
        d0[r] = rowsum16(dqdz * wa0);
        d1[r] = rowsum16(dqdz * wa1);
        qp[r] = rowsum16(fmaxf(z, 0.f) * w3);
      }
      if (i == 15) {
        *(f4*)(L.DP + 32 * w + 8 * g) = f4{d0.x, d1.x, d0.y, d1.y};
        *(f4*)(L.DP + 32 * w + 8 * g + 4) = f4{d0.z, d1.z, d0.w, d1.w};
        *(f4*)(L.QP + 16 * w + 4 * g) = qp;
      }
    }
    lds_sync32();
    // ---- phase 4: dL/dz3 of the lane's rows, dz2 = (dz3 W3) relu'(h2) of unit u
    {
      f4 s01 = {0.f, 0.f, 0.f, 0.f}, s23 = {0.f, 0.f, 0.f, 0.f}, qs = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int v = 0; v < 8; ++v) {
        s01 += *(const f4*)(L.DP + 32 * v + 8 * g);
        s23 += *(const f4*)(L.DP + 32 * v + 8 * g + 4);
        qs += *(const f4*)(L.QP + 16 * v + 4 * g);
      }
      const float da0[4] = {s01.x, s01.z, s23.x, s23.z}, da1[4] = {s01.y, s01.w, s23.y, s23.w};
      const float w30 = TLa[kT3 + u], w31 = TLa[kT3 + kH2 + u];
      f4 dz;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float z0 = -loss_scale * da0[r] * (1.f - a0[r] * a0[r]);
        const float z1 = -loss_scale * da1[r] * (1.f - a1[r] * a1[r]);
        if (w == 0 && i == 0) {
          gb30 += z0;
          gb31 += z1;
          if (row0 + 4 * g + r < B) qsum += TLc[kTB] + qs[r];
        }
        const float d = h2[r] > 0.f ? z0 * w30 + z1 * w31 : 0.f;
        dz[r] = d;
        L.DZ2[(4 * g + r) * kLdH2 + u] = d;
        gb2 += d;
        gw30 += z0 * h2[r];
        gw31 += z1 * h2[r];
      }
      *(f4*)(L.DZ2T + u * kLdT16 + 4 * g) = dz;
    }
    lds_sync32();
    // ---- phase 5
#pragma unroll
    for (int kt = 0; kt < 16; ++kt) gW2[kt] = g16_wgrad(gW2[kt], L.DZ2T, 16 * w, L.H1T, 16 * kt, lane);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = 16 * (w + 8 * j) + i;
      const f32x4 acc = g16_xw128(L.DZ2, kLdH2, A.W2, kALd, 16 * (w + 8 * j), lane);
      f4 d;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        d[r] = L.H1[(4 * g + r) * kLdH1 + n] > 0.f ? acc[r] : 0.f;
        gb1[j] += d[r];
      }
      *(f4*)(L.DZ1T + n * kLdT16 + 4 * g) = d;
    }
    lds_sync32();
    // ---- phase 6
#pragma unroll
    for (int j = 0; j < 2; ++j) gW1[j] = g16_wgrad(gW1[j], L.DZ1T, 16 * (w + 8 * j), L.ST, 0, lane);
    lds_sync32();
  }
  float* P = partial + (int64_t)blockIdx.x * kAP;
  const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4, u = 16 * w + i;
#pragma unroll
  for (int kt = 0; kt < 16; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) P[kPW2 + (16 * w + 4 * g + r) * kALd + 16 * kt + i] = gW2[kt][r];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (i < kIn) {
#pragma unroll
      for (int r = 0; r < 4; ++r) P[kPW1 + (16 * (w + 8 * j) + 4 * g + r) * kIn + i] = gW1[j][r];
    }
    float b = gb1[j] + __shfl_xor(gb1[j], 16, 64);
    b += __shfl_xor(b, 32, 64);
    if (g == 0) P[kPB1 + 16 * (w + 8 * j) + i] = b;
  }
  gb2 += __shfl_xor(gb2, 16, 64);
  gb2 += __shfl_xor(gb2, 32, 64);
  gw30 += __shfl_xor(gw30, 16, 64);
  gw30 += __shfl_xor(gw30, 32, 64);
  gw31 += __shfl_xor(gw31, 16, 64);
  gw31 += __shfl_xor(gw31, 32, 64);
  if (g == 0) {
    P[pB2(kALd) + u] = gb2;
    P[pW3(kALd) + u] = gw30;
    P[pW3(kALd) + kH2 + u] = gw31;
  }
  if (w == 0 && i == 0) {
    atomicAdd(&L.RED[0], gb30);
    atomicAdd(&L.RED[1], gb31);
    atomicAdd(&L.RED[2], qsum);
  }
  lds_sync32();
  if (threadIdx.x < 2) P[pB3(kALd, 2) + threadIdx.x] = L.RED[threadIdx.x];
  if (threadIdx.x == 0 && q_out) atomicAdd(q_out, L.RED[2]);
}

// ================================================================ sliced gradient kernels
// Small minibatches.  The kernels above give a 256-row
// minibatch 16 workgroups (one per 16-row tile), each running the whole
// phase chain on one CU at two waves per SIMD: MFMA-rate bound on 16 of 256
// CUs.  The sliced schedule splits layer 2 over kSlices workgroups per row
// tile (16 units each: RT x 8 workgroups, 128 at batch 256), two launches per
// step:
//   fwd (rt, s)  layer 1 of every net the step reads (all 256 units; the
//                critic's Dropout), then the slice's 16 layer-2 units with K
//                split over the 4 waves -> pre-activations z2 (no b2, no
//                action columns) [rt][net][row][unit] in the scratch buffer
//   bwd (rt, s)  per row, from all 128 units of z2 (read back: 8 KB per net
//                and row tile): q, mu', Q', y, dL/dq (critic) or mu, dQ/da,
//                dL/dz3 (actor); then the slice's dz2, its dW2 rows and its
//                b2 / action-column / W3 gradients; and the slice's share of
//                dz1 = dz2_s W2_s (dz1 is linear in dz2, the relu' and
//                Dropout masks are elementwise) -> dW1 / db1 contributions
//                written to a second partial buffer [RT * kSlices][3328]
//                that k_adam_flat sums for W1 and b1.
// Every partial entry is written by exactly one workgroup.  Block b is row
// tile b / 8, slice b % 8: slice s always lands on XCD s, whose L2 then holds
// that slice's W2 rows for every row tile.
constexpr int kSlices = 8, kSliceU = kH2 / kSlices;  // 16 units per slice
constexpr int kSlThreads = 256;                       // 4 waves: one per SIMD
constexpr int kZPlane = kR * kH2;                     // one net's z2 of a row tile
// LDS layouts of the sliced kernels, laid out against the gfx950 bank rules
// (MI355X_MICROARCH.md §LDS; VERDICT r05: conflict cycles were 100 / 61 / 91 %
// of the LDS instructions of fwd<1> / bwd<1> / fwd<2>).  They replaced padded
// row-major layouts (DESIGN §13 has the A/B); the arithmetic is the same either way.
// Every XOR below touches only bits 2-3 of the column (which 16-B slot of a
// fragment) and depends only on a lane's own row, so each lane computes its
// addresses once and the unrolled accesses differ by immediate offsets (a
// swizzle that mixed the unrolled indices in cost ~80 VALU per wave).
//   [16][16] tiles read as 16-B MFMA fragments (lane (i, g): row i, floats
//     4g..4g+3; ds_read_b128 serves 16 lanes per cycle over 64 banks): rows of
//     16 floats, the slot XORed with (row >> 1) & 3 -- every lane group of the
//     fragment read and of the 8-lane ds_write_b128 of a transposed row covers
//     16 (8) distinct slots.  Also the [256][16] transposed layer 1.
//   [16][260] layer-1 outputs (written one float per lane, rows 4g + r, the
//     two 16-lane rows of a half 1,040 floats = 16 banks apart; read as
//     fragments, row i): the slot XORed with f(row >> 2), f = 0, 1, 1, 0, which
//     puts the four 4-row blocks of a ds_read_b128 lane group on disjoint slots.
//   [16][128 + 16] z2 planes: the row reductions read rows r and r + 1 in one
//     32-lane half, 16 banks apart.
//   the forward's K-split partials [wave][row][unit]: row r at 16 (r + r / 4),
//     so rows 4 apart (lanes g and g + 1 of one store) sit 16 banks apart.
constexpr int kSlLdT = 16;
constexpr int kSlLdH = kLdH1;
constexpr int kLdZ = kH2 + 16;
constexpr int kSlRed = 20 * kSliceU;  // floats per wave
__device__ __forceinline__ int sl_tmask(int row) { return ((row >> 1) & 3) << 2; }
__device__ __forceinline__ int sl_t16(int row, int col) { return row * kSlLdT + (col ^ sl_tmask(row)); }
__device__ __forceinline__ int sl_hmask(int row) { return (((row >> 2) ^ (row >> 3)) & 1) << 2; }
__device__ __forceinline__ int sl_red(int row, int j) { return (row + (row >> 2)) * kSliceU + j; }
constexpr int kW1Part = kPW2;                         // W1 + b1: floats per contribution row
enum { kSlCriticY = 0, kSlCriticBoot = 1, kSlActor = 2 };
__host__ __device__ constexpr int sl_planes(int mode) { return mode == kSlCriticBoot ? 3 : (mode == kSlActor ? 2 : 1); }
// net p of a step: critic modes 0 critic, 1 target actor, 2 target critic;
// actor mode 0 actor, 1 critic
__host__ __device__ constexpr int sl_ld(int mode, int p) {
  return (mode == kSlActor && p == 0) || (mode == kSlCriticBoot && p == 1) ? kALd : kCLd;
}
__host__ __device__ constexpr int sl_nout(int mode, int p) { return sl_ld(mode, p) == kALd ? 2 : 1; }
constexpr size_t sl_fwd_lds(int) { return (size_t)(kR * kSlLdT + kR * kSlLdH + kH1 + 4 * kSlRed) * 4; }
constexpr size_t sl_bwd_lds(int mode) {
  return (size_t)(2 * kR * kSlLdT + sl_planes(mode) * (kR * kLdZ + 1024) + kR * kSlLdH + kH1 * kSlLdT +
                  3 * kSliceU * kSlLdT + 32 + 2 * kR + 2 * kR + kR + 4) *
         4;
}
static_assert(sl_fwd_lds(kSlCriticBoot) <= 160 * 1024 && sl_bwd_lds(kSlCriticBoot) <= 160 * 1024, "LDS budget");

// p[i] where ok, else 0, as one unconditional load (of p[0] where !ok) and a
// select: a load under a branch put its value through a phi copy that the
// waitcnt pass guarded with a vmcnt(0), a round trip of every load in flight
__device__ __forceinline__ float ld_or0(const float* __restrict__ p, int64_t i, bool ok) {
  const float v = p[ok ? i : 0];
  return ok ? v : 0.f;
}

// g16_l1 on the sliced layouts with the weights already loaded (w1_frag,
// sk_net32.hpp: the fragments are issued ahead of the staging barrier)
__device__ __forceinline__ f32x4 g16_l1w(const float* S, f4 w, int lane) {
  const int i = lane & 15, g = lane >> 4;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  return m16x4(*(const f4*)(S + sl_t16(i, 4 * g)), w, z);
}
// (n = 16 nt + i: n's masks are i's)
// l1_out on the sliced layouts
__device__ __forceinline__ void l1_out_sl(f32x4 acc, const float* tl, int nt, int lane, float* H, float* HT, bool drop,
                                          uint32_t bits4) {
  const int i = lane & 15, g = lane >> 4, n = 16 * nt + i;
  const float b = tl[kT1 + n];
  f4 z;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float v = fmaxf(acc[r] + b, 0.f);
    if (drop) v = (bits4 >> r) & 1u ? v * 1.25f : 0.f;
    z[r] = v;
    H[(4 * g + r) * kSlLdH + 16 * nt + (i ^ sl_hmask(4 * g))] = v;
  }
  if (HT) *(f4*)(HT + n * kSlLdT + (4 * g ^ sl_tmask(i))) = z;
}
// g16_wgrad on the sliced layouts
__device__ __forceinline__ f32x4 g16_wgrad_sl(f32x4 acc, const float* AT, int m0, const float* BT, int n0, int lane) {
  const int i = lane & 15, g = lane >> 4;
  const int c = 4 * g ^ sl_tmask(i);  // m0, n0: multiples of 16
  return m16x4(*(const f4*)(AT + (m0 + i) * kSlLdT + c), *(const f4*)(BT + (n0 + i) * kSlLdT + c), acc);
}

// The replay minibatch gathered inside the critic's first launch
// (sk_critic_grad_f32_sampled): skmlp::RingSample / ring_row (sk_mlp.hpp).
// Each workgroup reads its own rows' states from the ring; the (slice 0, net
// 0) workgroup of every row tile also writes its 16 rows into the sample
// buffers, which the second launch and the actor step read.
using skmlp::RingSample;
using skmlp::ring_row;

template <int MODE>
__global__ void __launch_bounds__(kSlThreads) k_grad_slice_fwd(const float* __restrict__ f0, const float* __restrict__ f1,
                                                              const float* __restrict__ f2, const float* __restrict__ Sg,
                                                              const float* __restrict__ S2g, int64_t B,
                                                              int64_t key_row0, uint64_t seed,
                                                              const int64_t* __restrict__ call_ctr,
                                                              float* __restrict__ Z, float* step_ctr, int n_steps,
                                                              RingSample rs) {
  constexpr int NP = sl_planes(MODE);
  extern __shared__ __attribute__((aligned(16))) float smem_sl[];
  float* sS = smem_sl;              // [16][16] (sl_t16)
  float* sH = sS + kR * kSlLdT;     // [16][260] layer-1 outputs (sl_hmask)
  float* sB1 = sH + kR * kSlLdH;    // [256]
  float* sRed = sB1 + kH1;          // [4 waves][16 rows][16 units] K-split partials (sl_red)
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, g = lane >> 4;
  // block = (row tile, net, slice), slice fastest
  const int b = blockIdx.x, s = b % kSlices, p = (b / kSlices) % NP, rt = b / (kSlices * NP);
  const int64_t row0 = (int64_t)rt * kR;
  if (b == 0 && tid < n_steps) step_ctr[tid] += 1.0f;  // Adam's step (read by k_adam_flat)
  const float* F = p == 0 ? f0 : (p == 1 ? f1 : f2);
  const int ld = (MODE == kSlActor && p == 0) || (MODE == kSlCriticBoot && p == 1) ? kALd : kCLd;
  const float* Ssrc = MODE == kSlCriticBoot && p > 0 ? S2g : Sg;
  const bool drop = MODE != kSlActor && p == 0;
  // the ring's insert count first: the row draw (Philox) needs it, and issued
  // after the weight fragments it made the draw wait for all of them
  const int64_t t_total = rs.ring ? *rs.total : 0;
  const float bv = F[kPB1 + tid];  // b1, with the weight fragments
  // the slice's W2 fragments, rows 16 s + i, k = 64 w + 16 t + 4 g, and the
  // layer-1 fragments of n-tiles w + 4q: in flight under the staging
  f4 wv[4], w1v[4];
  {
    const gfp wr = (gfp)F + kPW2 + (size_t)(kSliceU * s + i) * ld + 64 * w + 4 * g;
#pragma unroll
    for (int t = 0; t < 4; ++t) wv[t] = *(gf4u)(wr + 16 * t);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) w1v[q] = w1_frag((gfp)F + kPW1, 16 * (w + 4 * q), lane);
  const int si = tid >> 4, sk = tid & 15;
  float sv;
  f4 rowv = {0.f, 0.f, 0.f, 0.f};
  bool scat = false;
  if (rs.ring) {
    const int64_t b = row0 + si, t = t_total;
    const bool ok = b < B && t > 0;
    const int64_t idx = ok ? ring_row(rs, b, t) : 0;
    const float* src = rs.ring + idx * 28;
    sv = ld_or0(src, (MODE == kSlCriticBoot && p > 0 ? 15 : 0) + sk, ok && sk < kIn);
    // the row into the sample buffers (stored after the barrier below, so no
    // wait for the sample's operands also waits for these stores)
    scat = ok && s == 0 && p == 0 && sk < 7;
    rowv = *(const f4*)(src + 4 * (sk < 7 ? sk : 0));
  } else {
    sv = ld_or0(Ssrc, (row0 + si) * kIn + sk, sk < kIn && row0 + si < B);
  }
  uint32_t keep0 = 0, keep1 = 0;
  if (drop) {
    const uint64_t call = (uint64_t)*call_ctr;
    keep0 = dropout_bits16(seed, call, key_row0 + row0, w, lane);      // n-tiles w, w + 8
    keep1 = dropout_bits16(seed, call, key_row0 + row0, w + 4, lane);  // n-tiles w + 4, w + 12
  }
  sS[sl_t16(si, sk)] = sv;
  sB1[tid] = bv;
  lds_sync32();
  if (scat) {
#pragma unroll
    for (int c = 0; c < 4; ++c) skmlp::ring_scatter(rs, row0 + si, 4 * sk + c, rowv[c]);
  }
  // ---- layer 1, n-tiles w, w + 4, w + 8, w + 12
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t bits = ((q & 1) ? keep1 : keep0) >> (4 * (q >> 1));
    l1_out_sl(g16_l1w(sS, w1v[q], lane), sB1, w + 4 * q, lane, sH, nullptr, drop, bits);
  }
  lds_sync32();
  // ---- layer 2 of the slice: wave w contracts inputs 64 w .. 64 w + 63
  {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const float* xr = sH + i * kSlLdH + 64 * w + (4 * g ^ sl_hmask(i));
#pragma unroll
    for (int t = 0; t < 4; ++t) acc = m16x4(*(const f4*)(xr + 16 * t), wv[t], acc);
    float* red = sRed + w * kSlRed + sl_red(4 * g, i);
#pragma unroll
    for (int r = 0; r < 4; ++r) red[r * kSliceU] = acc[r];
  }
  lds_sync32();
  // ---- z2[row][16 s + j] = the 4 waves' partials (thread = (row, j))
  {
    const int row = tid >> 4, j = tid & 15;
    const float* red = sRed + sl_red(row, j);
    const float z = (red[0] + red[kSlRed]) + (red[2 * kSlRed] + red[3 * kSlRed]);
    Z[((int64_t)rt * NP + p) * kZPlane + row * kH2 + kSliceU * s + j] = z;
  }
}

// sum over the 16 lanes of a DPP row, in every lane of the row (xor 1, xor 2,
// half-row mirror, row mirror: each step adds a lane-symmetric pair, so every
// lane ends with the same bits)
template <int CTRL>
__device__ __forceinline__ float dpp_all(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float rowall16(float v) {
  v += dpp_all<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_all<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_all<0x141>(v);  // row_half_mirror
  v += dpp_all<0x140>(v);  // row_mirror
  return v;
}


// The backward launch's workgroup `bid` (row tile bid / kSlices, slice
// bid % kSlices) on the LDS at smem_sl (sl_bwd_lds(MODE) bytes): the body of
// k_grad_slice_bwd, and of k_bwd_act_step32's backward workgroups.
#define SK_SLICE_BWD_PARAMS                                                                                      \
  const float *__restrict__ f0, const float *__restrict__ f1, const float *__restrict__ f2,                       \
      const float *__restrict__ Sg, const float *__restrict__ Ag, const float *__restrict__ Yg,                  \
      const float *__restrict__ Rg, const float *__restrict__ Dg, float gamma, int64_t B, int64_t key_row0,      \
      float scale, uint64_t seed, const int64_t *__restrict__ call_ctr, const float *__restrict__ Z,             \
      float *__restrict__ partial, float *__restrict__ partial_w1, float *__restrict__ stat_out,                 \
      uint8_t *__restrict__ mask_out
#define SK_SLICE_BWD_ARGS \
  f0, f1, f2, Sg, Ag, Yg, Rg, Dg, gamma, B, key_row0, scale, seed, call_ctr, Z, partial, partial_w1, stat_out, mask_out

// The backward of a (row tile, slice) in kBwdH = 2 workgroups: half hq
// owns n-tiles w + 4q for q = hq, hq + 2 (layer 1 of the trained net, the
// dW2 columns, the dz1 share and its dW1 / db1 contributions), each half
// redoing the loads, the per-row reductions and dz2 that both need.  Every
// output entry is computed by exactly one workgroup with the same operations
// in the same order as by a single workgroup, so the results are the same
// bits; the launch has twice the workgroups on the 256 CUs its 128 left half
// idle.  (One and four workgroups were measured and dropped: DESIGN §13.)
constexpr int kBwdH = 2, kBwdQ = 2;  // workgroups per (row tile, slice); n-tiles w + 4q per workgroup

template <int MODE>
__device__ __forceinline__ void grad_slice_bwd(int bid, float* smem_sl, SK_SLICE_BWD_PARAMS) {
  constexpr int NP = sl_planes(MODE);
  constexpr bool CRIT = MODE != kSlActor;
  constexpr int LD0 = sl_ld(MODE, 0), NPAR = CRIT ? kCP : kAP;
  float* sS = smem_sl;                  // [16][16] (sl_t16)
  float* sST = sS + kR * kSlLdT;        // [16 features][16 rows] (sl_t16)
  float* sZ = sST + kR * kSlLdT;        // [NP][16][kLdZ]
  float* sTL = sZ + NP * kR * kLdZ;     // [NP][1024] the nets' fp32 tails
  float* sH1 = sTL + NP * 1024;         // [16][260] layer 1 of the trained net, after Dropout (sl_hmask)
  float* sH1T = sH1 + kR * kSlLdH;      // [256][16] (sl_t16)
  float* sDZ2 = sH1T + kH1 * kSlLdT;    // [16 rows][16 slice units] (sl_t16)
  float* sDZ2T = sDZ2 + kSliceU * kSlLdT;  // [16 units][16 rows] (sl_t16)
  float* sH2T = sDZ2T + kSliceU * kSlLdT;  // [4 waves][16 units][4] per-unit gradient sums
  float* sA = sH2T + kSliceU * kSlLdT;  // [16][2] actions (critic)
  float* sRD = sA + 32;                 // [16] r or y, [16] done
  float* sDQ = sRD + 2 * kR;            // [16][2] dL/dq (critic) or dL/dz3 (actor)
  float* sST8 = sDQ + 2 * kR;           // [16] per-row e^2 (critic) or Q (actor)
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, g = lane >> 4;
  // block = (row tile, half, slice), slice fastest (slice s on XCD s)
  const int s = bid % kSlices, hq = (bid / kSlices) % kBwdH, rt = bid / (kSlices * kBwdH);
  const int64_t row0 = (int64_t)rt * kR;
  const float* fl[3] = {f0, f1, f2};
  const gfp W2 = (gfp)f0 + kPW2;
  TP32(20);
  // ---- phase 0: every global load; the tails first, their index arithmetic
  // ahead of every load (after the others it shared registers with loads in
  // flight and cost a full vmcnt(0) round trip)
  float tv[NP][4];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int k = 0; k < 4; ++k) tv[p][k] = tail_src((gfp)fl[p], sl_ld(MODE, p), sl_nout(MODE, p), tid + kSlThreads * k);
  // the slice's W2 rows down the columns of n-tiles w + 4q (the dz1 GEMM of
  // phase 3), q = hq + kBwdH k: this workgroup's n-tiles
  float wd[kBwdQ][4];
#pragma unroll
  for (int k = 0; k < kBwdQ; ++k)
#pragma unroll
    for (int c = 0; c < 4; ++c)
      wd[k][c] = W2[(size_t)(kSliceU * s + 4 * g + c) * LD0 + 16 * (w + 4 * (hq + kBwdH * k)) + i];
  f4 w1v[kBwdQ];
#pragma unroll
  for (int k = 0; k < kBwdQ; ++k) w1v[k] = w1_frag((gfp)f0 + kPW1, 16 * (w + 4 * (hq + kBwdH * k)), lane);
  f4 zv[NP][2];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int m = 0; m < 2; ++m)
      zv[p][m] = *(const f4*)(Z + ((int64_t)rt * NP + p) * kZPlane + 4 * (tid + kSlThreads * m));
  const int si = tid >> 4, sk = tid & 15;
  const float sv = ld_or0(Sg, (row0 + si) * kIn + sk, sk < kIn && row0 + si < B);
  const bool rok = tid < kR && row0 + tid < B;
  const float av = CRIT && tid < 32 && row0 + (tid >> 1) < B ? Ag[row0 * 2 + tid] : 0.f;
  const float rv = CRIT && rok ? (MODE == kSlCriticBoot ? Rg[row0 + tid] : Yg[row0 + tid]) : 0.f;
  const float dv = MODE == kSlCriticBoot && rok ? Dg[row0 + tid] : 0.f;
  // keep0: n-tiles w, w + 8 (q = 0, 2); keep1: w + 4, w + 12 (q = 1, 3)
  uint32_t keep0 = 0, keep1 = 0;
  if (CRIT) {
    const uint64_t call = (uint64_t)*call_ctr;
    // (this workgroup's q = hq + kBwdH k all share hq's parity)
    if ((hq & 1) == 0) keep0 = dropout_bits16(seed, call, key_row0 + row0, w, lane);
    if ((hq & 1) == 1) keep1 = dropout_bits16(seed, call, key_row0 + row0, w + 4, lane);
  }
  sS[sl_t16(si, sk)] = sv;
  sST[sl_t16(sk, si)] = sv;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int q = tid + kSlThreads * m;
      *(f4*)(sZ + p * kR * kLdZ + (q >> 5) * kLdZ + 4 * (q & 31)) = zv[p][m];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) sTL[p * 1024 + tid + kSlThreads * k] = tv[p][k];
  }
  if (CRIT && tid < 32) sA[tid] = av;
  if (CRIT && tid < kR) {
    sRD[tid] = rv;
    sRD[kR + tid] = dv;
  }
  if (CRIT && mask_out && s == 0) {
#pragma unroll
    for (int k = 0; k < kBwdQ; ++k) {
      const int q = hq + kBwdH * k;
      const uint32_t bits = ((q & 1) ? keep1 : keep0) >> (4 * (q >> 1));
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (row0 + 4 * g + r < B) mask_out[(row0 + 4 * g + r) * kH1 + 16 * (w + 4 * q) + i] = (bits >> r) & 1u;
    }
  }
  lds_sync32();
  TP32(21);
  // ---- phase 1: layer 1 of the trained net (MFMA) and the per-row reductions (VALU)
#pragma unroll
  for (int k = 0; k < kBwdQ; ++k) {
    const int q = hq + kBwdH * k, nt = w + 4 * q;
    const uint32_t bits = ((q & 1) ? keep1 : keep0) >> (4 * (q >> 1));
    l1_out_sl(g16_l1w(sS, w1v[k], lane), sTL, nt, lane, sH1, sH1T, CRIT, bits);
  }
  {
    const int row = tid >> 4, c = tid & 15;
    const bool valid = row0 + row < B;
    const float* T0 = sTL;
    const float* T1 = sTL + 1024;
    const float* z0 = sZ + row * kLdZ;
    if (CRIT) {
      const float a0 = sA[2 * row], a1 = sA[2 * row + 1];
      float y;
      if (MODE == kSlCriticBoot) {
        const float* za = sZ + kR * kLdZ + row * kLdZ;
        const float* zt = sZ + 2 * kR * kLdZ + row * kLdZ;
        const float* T2 = sTL + 2048;
        float m0 = 0.f, m1 = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int u = c + 16 * k;
          const float h = fmaxf(za[u] + T1[kT2 + u], 0.f);
          m0 += h * T1[kT3 + u];
          m1 += h * T1[kT3 + kH2 + u];
        }
        const float mu0 = tanhf(rowall16((m0)) + T1[kTB]);
        const float mu1 = tanhf(rowall16((m1)) + T1[kTB + 1]);
        float qt = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int u = c + 16 * k;
          qt += fmaxf(zt[u] + T2[kT2 + u] + T2[kTA + 2 * u] * mu0 + T2[kTA + 2 * u + 1] * mu1, 0.f) * T2[kT3 + u];
        }
        y = sRD[row] + gamma * (1.f - sRD[kR + row]) * (T2[kTB] + rowall16((qt)));
      } else {
        y = sRD[row];
      }
      float qc = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int u = c + 16 * k;
        qc += fmaxf(z0[u] + T0[kT2 + u] + T0[kTA + 2 * u] * a0 + T0[kTA + 2 * u + 1] * a1, 0.f) * T0[kT3 + u];
      }
      qc = rowsum16(qc);
      if (c == 15) {
        const float e = valid ? qc + T0[kTB] - y : 0.f;
        sDQ[2 * row] = scale * e;
        sST8[row] = e * e;
      }
    } else {
      const float* zc = sZ + kR * kLdZ + row * kLdZ;
      float m0 = 0.f, m1 = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int u = c + 16 * k;
        const float h = fmaxf(z0[u] + T0[kT2 + u], 0.f);
        m0 += h * T0[kT3 + u];
        m1 += h * T0[kT3 + kH2 + u];
      }
      const float mu0 = tanhf(rowall16((m0)) + T0[kTB]);
      const float mu1 = tanhf(rowall16((m1)) + T0[kTB + 1]);
      float d0 = 0.f, d1 = 0.f, qs = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int u = c + 16 * k;
        const float wa0 = T1[kTA + 2 * u], wa1 = T1[kTA + 2 * u + 1], w3 = T1[kT3 + u];
        const float z = zc[u] + T1[kT2 + u] + wa0 * mu0 + wa1 * mu1;
        const float dq = z > 0.f ? w3 : 0.f;
        d0 += dq * wa0;
        d1 += dq * wa1;
        qs += fmaxf(z, 0.f) * w3;
      }
      d0 = rowsum16(d0);
      d1 = rowsum16(d1);
      qs = rowsum16(qs);
      if (c == 15) {
        sDQ[2 * row] = valid ? -scale * d0 * (1.f - mu0 * mu0) : 0.f;
        sDQ[2 * row + 1] = valid ? -scale * d1 * (1.f - mu1 * mu1) : 0.f;
        sST8[row] = valid ? qs + T1[kTB] : 0.f;
      }
    }
  }
  lds_sync32();
  TP32(22);
  // ---- phase 2: dz2 of the slice's units (thread = (row, j))
  {
    const int row = tid >> 4, j = tid & 15, u = kSliceU * s + j;
    const float* T0 = sTL;
    float dz, h2x;
    if (CRIT) {
      const float z = sZ[row * kLdZ + u] + T0[kT2 + u] + T0[kTA + 2 * u] * sA[2 * row] + T0[kTA + 2 * u + 1] * sA[2 * row + 1];
      const float h2 = fmaxf(z, 0.f), dq = sDQ[2 * row];
      dz = h2 > 0.f ? dq * T0[kT3 + u] : 0.f;
      h2x = dq * h2;
    } else {
      const float h2 = fmaxf(sZ[row * kLdZ + u] + T0[kT2 + u], 0.f);
      dz = h2 > 0.f ? sDQ[2 * row] * T0[kT3 + u] + sDQ[2 * row + 1] * T0[kT3 + kH2 + u] : 0.f;
      h2x = h2;
    }
    sDZ2[sl_t16(row, j)] = dz;
    sDZ2T[sl_t16(j, row)] = dz;
    // the unit's b2 and W3 (and, critic, action-column) gradients over the
    // wave's 4 rows (lanes j, j + 16, j + 32, j + 48), then across waves in phase 3
    float v[4];
    if (CRIT) {
      v[0] = dz;
      v[1] = dz * sA[2 * row];
      v[2] = dz * sA[2 * row + 1];
      v[3] = h2x;
    } else {
      v[0] = dz;
      v[1] = sDQ[2 * row] * h2x;
      v[2] = sDQ[2 * row + 1] * h2x;
      v[3] = 0.f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[k] += __shfl_xor(v[k], 16, 64);
      v[k] += __shfl_xor(v[k], 32, 64);
    }
    if (lane < kSliceU) *(f4*)(sH2T + (w * kSliceU + j) * 4) = f4{v[0], v[1], v[2], v[3]};
  }
  lds_sync32();
  TP32(23);
  // ---- phase 3: the slice's per-unit gradients; dW2 rows; dz1 share -> dW1, db1
  float* P = partial + (int64_t)rt * NPAR;
  float* PW = partial_w1 + (int64_t)(rt * kSlices + s) * kW1Part;  // one contribution row per (row tile, slice)
  if (hq != 0) {
    // the slice's per-unit gradients and b3 / the stat: half 0's
  } else if (tid < kSliceU) {
    const int j = tid, u = kSliceU * s + j;
    const f4 v = (*(const f4*)(sH2T + j * 4) + *(const f4*)(sH2T + (kSliceU + j) * 4)) +
                 (*(const f4*)(sH2T + (2 * kSliceU + j) * 4) + *(const f4*)(sH2T + (3 * kSliceU + j) * 4));
    const float b2 = v.x, x0 = v.y, x1 = v.z, x3 = v.w;
    if (CRIT) {
      P[pB2(kCLd) + u] = b2;
      P[skpart::critic_w2_action(u, 0)] = x0;
      P[skpart::critic_w2_action(u, 1)] = x1;
      P[pW3(kCLd) + u] = x3;
    } else {
      P[pB2(kALd) + u] = b2;
      P[pW3(kALd) + u] = x0;
      P[pW3(kALd) + kH2 + u] = x1;
    }
  } else if (s == 0 && tid == 64) {  // a lane of wave 1: b3 and the step's loss / Q sum
    float b30 = 0.f, b31 = 0.f, st = 0.f;
#pragma unroll
    for (int r = 0; r < kR; ++r) {
      b30 += sDQ[2 * r];
      b31 += sDQ[2 * r + 1];
      st += sST8[r];
    }
    if (CRIT) {
      P[pB3(kCLd, 1)] = b30;
    } else {
      P[pB3(kALd, 2)] = b30;
      P[pB3(kALd, 2) + 1] = b31;
    }
    if (stat_out) atomicAdd(stat_out, st);
  }
  const float dscale = CRIT ? 1.25f : 1.f;  // Dropout(0.2): kept activations x 1.25
  const f4 dzr = *(const f4*)(sDZ2 + sl_t16(i, 4 * g));
  const f4 sT = *(const f4*)(sST + sl_t16(i, 4 * g));
#pragma unroll
  for (int k = 0; k < kBwdQ; ++k) {
    const int q = hq + kBwdH * k, nt = w + 4 * q, n = 16 * nt + i;
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    const f32x4 gw2 = g16_wgrad_sl(z4, sDZ2T, 0, sH1T, 16 * nt, lane);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = kSliceU * s + 4 * g + r;
      P[CRIT ? skpart::critic_w2_main(o, n) : kPW2 + o * kALd + n] = gw2[r];
    }
    const f32x4 acc = m16x4(dzr, f4{wd[k][0], wd[k][1], wd[k][2], wd[k][3]}, z4);
    f4 d;
    float b = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      d[r] = sH1[(4 * g + r) * kSlLdH + 16 * nt + (i ^ sl_hmask(4 * g))] > 0.f ? acc[r] * dscale : 0.f;
      b += d[r];
    }
    b += __shfl_xor(b, 16, 64);
    b += __shfl_xor(b, 32, 64);
    if (g == 0) PW[kPB1 + n] = b;
    const f32x4 gw1 = m16x4(d, sT, z4);
    if (i < kIn) {
#pragma unroll
      for (int r = 0; r < 4; ++r) PW[kPW1 + (16 * nt + 4 * g + r) * kIn + i] = gw1[r];
    }
  }
  TP32(24);
}

template <int MODE>
__global__ void __launch_bounds__(kSlThreads) k_grad_slice_bwd(SK_SLICE_BWD_PARAMS) {
  extern __shared__ __attribute__((aligned(16))) float smem_sl[];
  grad_slice_bwd<MODE>(blockIdx.x, smem_sl, SK_SLICE_BWD_ARGS);
}

// A gradient step's backward launch with the next acting tick beside it
// (the fused overlapped learner tick: sk_critic_grad_f32_sampled_step carries
// it in the critic's backward, sk_actor_grad_f32_step in the actor's):
// workgroups [0, GA) run act_step32 (k_act_step32's 16 games each), the rest
// grad_slice_bwd<MODE> (k_grad_slice_bwd's workgroup blockIdx - GA).  The
// two share no data: the backward reads the minibatch, the nets and the
// forward's z2; the acting half reads the actor and the observations and
// writes the env, the actions and the ring (the minibatch was gathered
// before, excluding the rows this insert writes).  LDS is the larger of the
// two layouts: two workgroups per CU (the critic's 78,544 B twice fill the
// CU's 160 KiB).
constexpr size_t bwd_act_lds(int mode) { return kActStepLds > sl_bwd_lds(mode) ? kActStepLds : sl_bwd_lds(mode); }
static_assert(2 * bwd_act_lds(kSlCriticBoot) <= 160 * 1024 && 2 * bwd_act_lds(kSlActor) <= 160 * 1024,
              "two fused workgroups per CU");
static_assert(kSlThreads == kFwdThreads, "one workgroup size for both halves");
template <int MODE, bool NOISE>
__global__ void __launch_bounds__(kFwdThreads) k_bwd_act_step32(SK_SLICE_BWD_PARAMS, unsigned GA,
                                                                const float* __restrict__ aflat,
                                                                const char* __restrict__ apack,
                                                                float* __restrict__ act_out, float sd, float action_sd,
                                                                uint64_t aseed, uint64_t* __restrict__ acall_ctr,
                                                                sk::StepArgs a, sk::Cfg c) {
  extern __shared__ __attribute__((aligned(16))) float smem_sl[];
  if (blockIdx.x < GA) {
    act_step32<NOISE>(aflat, apack, act_out, sd, action_sd, aseed, acall_ctr, a, c, (char*)smem_sl, GA);
  } else {
    grad_slice_bwd<MODE>((int)(blockIdx.x - GA), smem_sl, SK_SLICE_BWD_ARGS);
  }
}

int64_t subtiles_per_wg32(int64_t B) {  // 16-row sub-tiles; <= 256 workgroups, >= 1 sub-tile each
  const int64_t tiles = (B + kR - 1) / kR;
  return (tiles + 255) / 256;
}

// the sliced schedule: automatic up to kSliceMaxTiles row tiles (batch 512);
// SK_SLICE32=0 never, =1 at every batch (A/B and tests)
constexpr int64_t kSliceMaxTiles = 32;
int slice_env() {  // read at every call: tests switch it per case
  const char* e = getenv("SK_SLICE32");
  return e && *e ? atoi(e) : -1;
}

template <int MODE>
int launch_sliced(const float* f0, const float* f1, const float* f2, const float* S, const float* S2,
                  const float* A, const float* Y, const float* R, const float* D, float gamma, int64_t B,
                  int64_t key_row0, float scale, uint64_t seed, const int64_t* call_ctr, float* partials,
                  float* scratch, int64_t w1_rows, float* step_ctr, int n_steps, float* stat_out, uint8_t* mask_out,
                  hipStream_t st, RingSample rs = RingSample{}, const sk::ActStepJob* job = nullptr) {
  static bool attr = false;
  if (!attr) {
    set_lds32(k_grad_slice_fwd<MODE>, sl_fwd_lds(MODE));
    set_lds32(k_grad_slice_bwd<MODE>, sl_bwd_lds(MODE));
    set_lds32(k_bwd_act_step32<MODE, true>, bwd_act_lds(MODE));
    set_lds32(k_bwd_act_step32<MODE, false>, bwd_act_lds(MODE));
    attr = true;
  }
  float* Z = scratch + w1_rows * kW1Part;
  const unsigned G = (unsigned)w1_rows;  // row tiles x slices
  k_grad_slice_fwd<MODE><<<G * sl_planes(MODE), kSlThreads, sl_fwd_lds(MODE), st>>>(f0, f1, f2, S, S2, B, key_row0, seed, call_ctr, Z,
                                                                  step_ctr, n_steps, rs);
  if (job) {  // the acting tick's workgroups first, then the backward's
    sk::StepArgs a = job->a;
    const unsigned GA = (unsigned)((a.n + 15) / 16);
    a.grid_blocks = GA;
    constexpr size_t lds = bwd_act_lds(MODE);
    if (job->sd != 0.f)
      k_bwd_act_step32<MODE, true><<<GA + G * kBwdH, kFwdThreads, lds, st>>>(
          f0, f1, f2, S, A, Y, R, D, gamma, B, key_row0, scale, seed, call_ctr, Z, partials, scratch, stat_out,
          mask_out, GA, job->aflat, job->apack, job->act_out, job->sd, job->action_sd, job->seed, job->call_ctr, a,
          job->c);
    else
      k_bwd_act_step32<MODE, false><<<GA + G * kBwdH, kFwdThreads, lds, st>>>(
          f0, f1, f2, S, A, Y, R, D, gamma, B, key_row0, scale, seed, call_ctr, Z, partials, scratch, stat_out,
          mask_out, GA, job->aflat, job->apack, job->act_out, 0.f, job->action_sd, job->seed, job->call_ctr, a,
          job->c);
    return hipGetLastError() == hipSuccess ? SK_OK : SK_EHIP;
  }
  k_grad_slice_bwd<MODE><<<G * kBwdH, kSlThreads, sl_bwd_lds(MODE), st>>>(f0, f1, f2, S, A, Y, R, D, gamma, B, key_row0,
                                                                  scale, seed, call_ctr, Z, partials, scratch,
                                                                  stat_out, mask_out);
  return hipGetLastError() == hipSuccess ? SK_OK : SK_EHIP;
}

}  // namespace

// csrc/sk_replay.hip
int replay_sample_excl(const float* ring, int64_t capacity, const int64_t* total, uint64_t seed, int32_t draw,
                       int64_t batch, float* s, float* a, float* r, float* s2, float* d, int64_t excl,
                       hipStream_t stream);

extern "C" {

int64_t sk_update_scratch_f32(int64_t batch, int64_t* w1_rows) {
  int64_t rows = 0, floats = 0;
  if (batch > 0 && batch <= ((int64_t)1 << 30)) {
    const int64_t RT = (batch + kR - 1) / kR;
    const int m = slice_env();
    if (m == 1 || (m != 0 && RT <= kSliceMaxTiles)) {
      rows = RT * kSlices;
      floats = rows * kW1Part + RT * 3 * kZPlane;
    }
  }
  if (w1_rows) *w1_rows = rows;
  return floats;
}

int64_t sk_update_partials_f32(int64_t batch) {
  if (batch <= 0) return 0;
  if (sk_update_scratch_f32(batch, nullptr) > 0) return (batch + kR - 1) / kR;  // sliced: one row per row tile
  const int64_t spw = subtiles_per_wg32(batch);
  return ((batch + kR - 1) / kR + spw - 1) / spw;
}

static int critic_f32(const float* critic_flat, const float* obs, const float* actions, const float* targets,
                      const float* next_obs, const float* rewards, const float* done, float gamma,
                      const float* target_actor_flat, const float* target_critic_flat, int64_t batch,
                      int64_t row_offset, float grad_scale, uint64_t seed, const int64_t* call_counter,
                      float* partials, float* step_counters, int32_t n_steps, float* loss_sum,
                      uint8_t* dropout_mask, float* scratch, const sk::ActStepJob* job, void* stream) {
  const bool boot = target_actor_flat != nullptr;
  if (boot && (!target_critic_flat || !next_obs || !rewards || !done)) return SK_EINVAL;
  if (!boot && !targets) return SK_EINVAL;
  if (!critic_flat || !obs || !actions || !call_counter || !partials || batch <= 0) return SK_EINVAL;
  if (row_offset < 0 || (row_offset & 3)) return SK_EINVAL;
  if ((n_steps > 0 && !step_counters) || n_steps < 0 || n_steps > 64) return SK_EINVAL;
  int64_t w1_rows = 0;
  if (sk_update_scratch_f32(batch, &w1_rows) > 0) {
    if (!scratch) return SK_EINVAL;
    if (boot)
      return launch_sliced<kSlCriticBoot>(critic_flat, target_actor_flat, target_critic_flat, obs, next_obs, actions,
                                          nullptr, rewards, done, gamma, batch, row_offset, grad_scale, seed,
                                          call_counter, partials, scratch, w1_rows, step_counters, n_steps, loss_sum,
                                          dropout_mask, (hipStream_t)stream, RingSample{}, job);
    return launch_sliced<kSlCriticY>(critic_flat, nullptr, nullptr, obs, nullptr, actions, targets, nullptr, nullptr,
                                     0.f, batch, row_offset, grad_scale, seed, call_counter, partials, scratch,
                                     w1_rows, step_counters, n_steps, loss_sum, dropout_mask, (hipStream_t)stream,
                                     RingSample{}, job);
  }
  static bool attr = false;
  if (!attr) {
    set_lds32(k_critic_grad32<true>, kLdsGrad32);
    set_lds32(k_critic_grad32<false>, kLdsGrad32);
    attr = true;
  }
  const int64_t spw = subtiles_per_wg32(batch);
  const unsigned G = (unsigned)sk_update_partials_f32(batch);
  auto kern = boot ? k_critic_grad32<true> : k_critic_grad32<false>;
  kern<<<G, kThreads, kLdsGrad32, (hipStream_t)stream>>>(
      critic_flat, obs, actions, targets, batch, row_offset, (int)spw, grad_scale, seed, call_counter, partials,
      step_counters, n_steps, loss_sum, dropout_mask, next_obs, rewards, done, gamma, target_actor_flat,
      target_critic_flat);
  if (hipGetLastError() != hipSuccess) return SK_EHIP;
  if (!job) return SK_OK;
  return sk_launch_act_step32(job->aflat, job->apack, job->act_out, job->sd, job->action_sd, job->seed, job->call_ctr, job->a,
                              job->c, (hipStream_t)stream);
}

int sk_critic_grad_f32(const float* critic_flat, const float* obs, const float* actions, const float* targets,
                       const float* next_obs, const float* rewards, const float* done, float gamma,
                       const float* target_actor_flat, const float* target_critic_flat, int64_t batch,
                       int64_t row_offset, float grad_scale, uint64_t seed, const int64_t* call_counter,
                       float* partials, float* step_counters, int32_t n_steps, float* loss_sum,
                       uint8_t* dropout_mask, float* scratch, void* stream) {
  return critic_f32(critic_flat, obs, actions, targets, next_obs, rewards, done, gamma, target_actor_flat,
                    target_critic_flat, batch, row_offset, grad_scale, seed, call_counter, partials, step_counters,
                    n_steps, loss_sum, dropout_mask, scratch, nullptr, stream);
}

int sk_critic_grad_f32_step(const float* critic_flat, const float* obs, const float* actions, const float* targets,
                            const float* next_obs, const float* rewards, const float* done, float gamma,
                            const float* target_actor_flat, const float* target_critic_flat, int64_t batch,
                            int64_t row_offset, float grad_scale, uint64_t seed, const int64_t* call_counter,
                            float* partials, float* step_counters, int32_t n_steps, float* loss_sum,
                            uint8_t* dropout_mask, float* scratch, const sk_step_job* job, void* stream) {
  if (!job) return SK_EINVAL;
  sk::ActStepJob j;
  std::memcpy(&j, job, sizeof(j));
  if (j.magic != sk::kActStepJobMagic) return SK_EINVAL;
  return critic_f32(critic_flat, obs, actions, targets, next_obs, rewards, done, gamma, target_actor_flat,
                    target_critic_flat, batch, row_offset, grad_scale, seed, call_counter, partials, step_counters,
                    n_steps, loss_sum, dropout_mask, scratch, &j, stream);
}

static int critic_sampled(const float* critic_flat, const sk_ring_sample* q, float gamma,
                          const float* target_actor_flat, const float* target_critic_flat, int64_t batch,
                          int64_t row_offset, float grad_scale, uint64_t seed, const int64_t* call_counter,
                          float* partials, float* step_counters, int32_t n_steps, float* loss_sum,
                          uint8_t* dropout_mask, float* scratch, const sk::ActStepJob* job, void* stream) {
  if (!q || !q->ring || !q->total || !q->s || !q->a || !q->r || !q->s2 || !q->d || q->capacity <= 0) return SK_EINVAL;
  if (q->exclude < 0 || q->exclude >= q->capacity) return SK_EINVAL;  // as sk_replay_sample_excl
  if ((((uintptr_t)q->ring) & 15) || (((uintptr_t)q->s) & 15) || (((uintptr_t)q->s2) & 15) || (((uintptr_t)q->a) & 7))
    return SK_EINVAL;
  const bool boot = target_actor_flat != nullptr;
  if (boot && !target_critic_flat) return SK_EINVAL;
  if (!critic_flat || !call_counter || !partials || batch <= 0) return SK_EINVAL;
  if (row_offset < 0 || (row_offset & 3)) return SK_EINVAL;
  if ((n_steps > 0 && !step_counters) || n_steps < 0 || n_steps > 64) return SK_EINVAL;
  int64_t w1_rows = 0;
  if (sk_update_scratch_f32(batch, &w1_rows) > 0) {
    if (!scratch) return SK_EINVAL;
    const RingSample rs{q->ring, q->capacity, q->total, q->seed, q->draw, q->s, q->a, q->r, q->s2, q->d, q->exclude};
    if (boot)
      return launch_sliced<kSlCriticBoot>(critic_flat, target_actor_flat, target_critic_flat, q->s, q->s2, q->a,
                                          nullptr, q->r, q->d, gamma, batch, row_offset, grad_scale, seed,
                                          call_counter, partials, scratch, w1_rows, step_counters, n_steps, loss_sum,
                                          dropout_mask, (hipStream_t)stream, rs, job);
    return launch_sliced<kSlCriticY>(critic_flat, nullptr, nullptr, q->s, nullptr, q->a, q->r, nullptr, nullptr, 0.f,
                                     batch, row_offset, grad_scale, seed, call_counter, partials, scratch, w1_rows,
                                     step_counters, n_steps, loss_sum, dropout_mask, (hipStream_t)stream, rs, job);
  }
  // unsliced batches: the gather as its own launch
  const int rc = replay_sample_excl(q->ring, q->capacity, q->total, q->seed, q->draw, batch, q->s, q->a, q->r, q->s2,
                                    q->d, q->exclude, (hipStream_t)stream);
  if (rc != SK_OK) return rc;
  const int rc2 = sk_critic_grad_f32(critic_flat, q->s, q->a, boot ? nullptr : q->r, boot ? q->s2 : nullptr,
                                     boot ? q->r : nullptr, boot ? q->d : nullptr, gamma, target_actor_flat,
                                     target_critic_flat, batch, row_offset, grad_scale, seed, call_counter, partials,
                                     step_counters, n_steps, loss_sum, dropout_mask, scratch, stream);
  if (rc2 != SK_OK || !job) return rc2;
  return sk_launch_act_step32(job->aflat, job->apack, job->act_out, job->sd, job->action_sd, job->seed, job->call_ctr, job->a,
                              job->c, (hipStream_t)stream);
}

int sk_critic_grad_f32_sampled(const float* critic_flat, const sk_ring_sample* q, float gamma,
                               const float* target_actor_flat, const float* target_critic_flat, int64_t batch,
                               int64_t row_offset, float grad_scale, uint64_t seed, const int64_t* call_counter,
                               float* partials, float* step_counters, int32_t n_steps, float* loss_sum,
                               uint8_t* dropout_mask, float* scratch, void* stream) {
  return critic_sampled(critic_flat, q, gamma, target_actor_flat, target_critic_flat, batch, row_offset, grad_scale,
                        seed, call_counter, partials, step_counters, n_steps, loss_sum, dropout_mask, scratch, nullptr,
                        stream);
}

int sk_critic_grad_f32_sampled_step(const float* critic_flat, const sk_ring_sample* q, float gamma,
                                    const float* target_actor_flat, const float* target_critic_flat, int64_t batch,
                                    int64_t row_offset, float grad_scale, uint64_t seed,
                                    const int64_t* call_counter, float* partials, float* step_counters,
                                    int32_t n_steps, float* loss_sum, uint8_t* dropout_mask, float* scratch,
                                    const sk_step_job* job, void* stream) {
  if (!job) return SK_EINVAL;
  sk::ActStepJob j;
  std::memcpy(&j, job, sizeof(j));
  if (j.magic != sk::kActStepJobMagic) return SK_EINVAL;
  return critic_sampled(critic_flat, q, gamma, target_actor_flat, target_critic_flat, batch, row_offset, grad_scale,
                        seed, call_counter, partials, step_counters, n_steps, loss_sum, dropout_mask, scratch, &j,
                        stream);
}

int sk_actor_grad_f32(const float* actor_flat, const float* critic_flat, const float* obs, int64_t batch,
                      float loss_scale, float* partials, float* step_counters, int32_t n_steps, float* q_sum,
                      float* scratch, void* stream) {
  if (!actor_flat || !critic_flat || !obs || !partials || batch <= 0) return SK_EINVAL;
  if ((n_steps > 0 && !step_counters) || n_steps < 0 || n_steps > 64) return SK_EINVAL;
  int64_t w1_rows = 0;
  if (sk_update_scratch_f32(batch, &w1_rows) > 0) {
    if (!scratch) return SK_EINVAL;
    return launch_sliced<kSlActor>(actor_flat, critic_flat, nullptr, obs, nullptr, nullptr, nullptr, nullptr, nullptr,
                                   0.f, batch, 0, loss_scale, 0, nullptr, partials, scratch, w1_rows, step_counters,
                                   n_steps, q_sum, nullptr, (hipStream_t)stream);
  }
  static bool attr = false;
  if (!attr) {
    set_lds32(k_actor_grad32, kLdsGrad32);
    attr = true;
  }
  const int64_t spw = subtiles_per_wg32(batch);
  const unsigned G = (unsigned)sk_update_partials_f32(batch);
  k_actor_grad32<<<G, kThreads, kLdsGrad32, (hipStream_t)stream>>>(actor_flat, critic_flat, obs, batch, (int)spw,
                                                                  loss_scale, partials, step_counters, n_steps,
                                                                  q_sum);
  return hipGetLastError() == hipSuccess ? SK_OK : SK_EHIP;
}

int sk_actor_grad_f32_step(const float* actor_flat, const float* critic_flat, const float* obs, int64_t batch,
                           float loss_scale, float* partials, float* step_counters, int32_t n_steps, float* q_sum,
                           float* scratch, const sk_step_job* job, void* stream) {
  if (!job) return SK_EINVAL;
  sk::ActStepJob j;
  std::memcpy(&j, job, sizeof(j));
  if (j.magic != sk::kActStepJobMagic) return SK_EINVAL;
  if (!actor_flat || !critic_flat || !obs || !partials || batch <= 0) return SK_EINVAL;
  if ((n_steps > 0 && !step_counters) || n_steps < 0 || n_steps > 64) return SK_EINVAL;
  int64_t w1_rows = 0;
  if (sk_update_scratch_f32(batch, &w1_rows) > 0) {
    if (!scratch) return SK_EINVAL;
    return launch_sliced<kSlActor>(actor_flat, critic_flat, nullptr, obs, nullptr, nullptr, nullptr, nullptr, nullptr,
                                   0.f, batch, 0, loss_scale, 0, nullptr, partials, scratch, w1_rows, step_counters,
                                   n_steps, q_sum, nullptr, (hipStream_t)stream, RingSample{}, &j);
  }
  const int rc = sk_actor_grad_f32(actor_flat, critic_flat, obs, batch, loss_scale, partials, step_counters, n_steps,
                                   q_sum, scratch, stream);
  if (rc != SK_OK) return rc;
  return sk_launch_act_step32(j.aflat, j.apack, j.act_out, j.sd, j.action_sd, j.seed, j.call_ctr, j.a, j.c,
                              (hipStream_t)stream);
}

}  // extern "C"

#ifdef SK_TRACE32
// diagnostic builds only (not in include/skillshot.h): [2 wg][32 points][memtime, realtime]
extern "C" int sk_debug_trace32(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sk_trace32), sizeof(g_sk_trace32)) == hipSuccess ? SK_OK : SK_EHIP;
}
#endif
