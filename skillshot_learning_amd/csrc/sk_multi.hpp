// sk_multi.hpp — the multi-tick step's device code and its launchers:
//   n ticks per launch (sk_env_step_multi, sk_env_step_multi_obs;
//   SK_MULTI_*): the state makes its round trip through memory every tick,
//   the launch boundary is paid once
//     k_step_multi        one lane per game, step-only; between ticks the
//                         88-B exchange format or a packed 48-B form, the
//                         action slab a tick ahead in registers or through a
//                         feed wave and LDS
//     k_step_split_multi  two lanes per game, step-only or with obs / reward;
//                         optionally an action-slab prefetch wave; step-only
//                         also with the packed 48-B form between ticks (8 B
//                         per player and plane), the default from 40,960 to
//                         98,304 games, there in long launches on fp32 trig
//                         with the wave's exact fallback (FAST)
//                         The packed launch is peeled: tick 0 and the
//                         last tick on the generic tick, between them a
//                         steady loop that knows its state form at compile
//                         time (split_tick_carry's STEADY form), 32-bit
//                         offsets into the ring and the output rows, and
//                         (FAST) the tick's state-independent arithmetic
//                         under its loads (SplitPre), there also the lanes
//                         that may need the exact evaluation
//                         (split_pre_maybe: the exactness guard is one
//                         scalar branch behind the state wait), and a rest
//                         between its stores and its reload
//     both run the carried-sincos tick: tick_env_carry (sk_device.hpp) and
//     split_tick_carry (below)
//
// Part of sk_engine.hip's translation unit, not a header to share: the kernels
// keep their global-namespace names, so sk_engine.hip includes this file once,
// behind its own `using namespace sk;` and reward_of.  Which instantiation a
// launch runs is decided on the host in sk_multi_plan.hpp (plan_multi) and
// mapped onto the launchers at this file's end by sk_engine.hip (launch_plan).
#ifndef SK_MULTI_HPP
#define SK_MULTI_HPP

#include <hip/hip_runtime.h>

#include <cstdint>

#include "sk_device.hpp"
#include "sk_range.hpp"
#include "sk_step.hpp"

// the steady loop's rest between a tick's stores and the next tick's loads, in units of 64 cycles
// (k_step_split_multi).  7 while the collision test stood in front of the stores; with the test
// behind them the tail is longer by itself and the best rest drops to 3 (DESIGN 4.1, round 16;
// profiles/r16_rest_sweep.jsonl)
static constexpr int kSteadyRest = 3;
// the steady tick's chain, from the state wait to the last state store, at issue priority 1: the
// partner wave's work under its own loads no longer takes the chain's slots
// (profiles/r16_bench_ab.jsonl)
static constexpr bool kSteadyPrio = true;

// ------------------------------------------------------------------ multi-tick step
// k_step_multi: n_ticks learner ticks of the step-only contract (sk_env_step
// with obs/reward NULL, n_ticks times) in ONE launch, one lane per game.  Each
// wave loops over the ticks; every tick it loads its 64 games' state, reads
// that tick's action slab from the HBM ring, runs k_step's tick, writes done
// / winner and stores the state back — so the 193 B per env-step of the
// contract move every tick, as in one k_step launch per tick,
// but the dependent-dispatch boundary (~1.7 us, MI355X_MICROARCH.md
// "boundary") and the end-of-dispatch L2 write-back are paid once per launch
// instead of once per tick.  Games are independent (SkillshotGame.py:58-94
// is intra-game), so no wave waits for another: no grid barrier.  The RNG
// step of tick t is step0 + t, as n_ticks sk_env_step calls would use.
//
// State port (SK_MULTI_POLICY / the `POL` template):
//   0  plain loads / stores, as k_step (a wave's own stores stay in its XCD's
//      L2, so the next tick's reload is an L2 hit),
//   1  write-through: stores `sc1` (the line leaves L2 and is dropped,
//      MI355X_MICROARCH.md "stores of each flavour") and loads `sc1` (bypass
//      L1), so every tick's 176 state bytes cross the L2/fabric boundary like
//      k_step's between launches.  Through buffer instructions (the cache
//      policy is an operand and the compiler tracks the waits) over ONE
//      resource whose base is the lowest plane (the host checks that every
//      plane lies within 4 GiB of it): one resource per plane spilled SGPRs.
//
// Resident format between ticks.  The 88-B SoA of include/skillshot.h is the
// exchange format: every launch loads it at its first tick and stores it at
// its last.  In between, a wave whose games all fit keeps them in a packed
// 48-B form in a scratch buffer of the handle (`pack`: R double2[n]
// rotations, Q double2[n] projectile rotations, S int4[n] = per player
// {px, py, qx, qy as bytes; cooldown int8, age u8, and ticks u16 (player 1)
// or the flag byte qv1 | qv2 << 1 | live << 2 | winner << 3 (player 2)}).
// Every tick still loads and stores every game's state through the same
// port; only the encoding is narrower (48 + ~40 B move
// per game-tick instead of 88 + ~72, reported against the fixed 193 B
// contract).  Fits: positions 0..255 (the board is 250), cooldown -128..127,
// age 0..255, ticks 0..65535, valid / live bytes 0..1, winner 0..3 — always
// true under the step protocol after the first tick (shoot is attempted
// every tick, Player.py:78-89, so cooldown and age stay in 0..16); a wave
// with any lane outside keeps the 88-B form for the rest of the launch.
typedef int skb4i __attribute__((ext_vector_type(4)));
typedef int skb2i __attribute__((ext_vector_type(2)));
typedef double skb2d __attribute__((ext_vector_type(2)));

struct MultiArgs {
  View v;
  int64_t n;
  const float2* actions;  // ring: [ring][2][N] float2
  int64_t ring;           // slabs in the ring
  int64_t slab0;          // slab of tick 0 (< ring)
  int n_ticks;
  int steady32;           // the packed split kernel's steady loop may run (step_multi); in n_ticks' padding
  uint8_t* done;          // tick t writes done + t * out_stride (nullable)
  uint8_t* winner;        // same (nullable)
  int64_t out_stride;
  int tick_limit;
  int auto_reset;
  int random_positions;
  uint64_t seed;
  int64_t env_offset;
  StepRef step;
  sk_counters* ctr;
  const char* base;       // POL 1: the lowest plane; off[k] = plane k - base (pos, rot, qpos, qrot, qcdage, misc)
  uint32_t off[6];
  char* pack;             // the packed resident planes (48 B x n), or NULL: the 88-B form every tick
  // the full contract (sk_env_step_multi_obs; k_step_split_multi<POL, true>):
  // tick t writes output slab so = (out0 + t) % out_slabs of obs
  // [slab][2][N][12], reward [slab][2][N] and (stride out_stride) done /
  // winner.  The step-only entry point: out0 0, out_slabs n_ticks (so = t).
  float* obs;
  float* reward;
  int reward_kind;
  int64_t out0, out_slabs;
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t raw_rsrc(const void* base) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, -1, 0x00020000);
}

// store_env_q through the port: the projectile-rotation plane only where it
// changed (a projectile fired, or the game restarted) unless force_q (the
// previous tick's state was packed: this plane is stale)
template <int POL>
__device__ __forceinline__ void store_env_port(const MultiArgs& a, __amdgpu_buffer_rsrc_t r, int64_t i, const Env& e,
                                               double q_old0, double q_old1, bool force_q) {
  const unsigned f = (unsigned)(e.qvalid[0] & 0xff) | ((unsigned)(e.qvalid[1] & 0xff) << 8) |
                     ((unsigned)(e.live & 0xff) << 16) | ((unsigned)(e.winner & 0xff) << 24);
  const bool qrot_changed = force_q | (int)(__double_as_longlong(e.qrot[0]) != __double_as_longlong(q_old0)) |
                            (int)(__double_as_longlong(e.qrot[1]) != __double_as_longlong(q_old1));
  if constexpr (POL == 0) {
    a.v.pos[i] = make_int4(e.px[0], e.py[0], e.px[1], e.py[1]);
    a.v.rot[i] = make_double2(e.rot[0], e.rot[1]);
    a.v.qpos[i] = make_int4(e.qx[0], e.qy[0], e.qx[1], e.qy[1]);
    if (qrot_changed) a.v.qrot[i] = make_double2(e.qrot[0], e.qrot[1]);
    a.v.qcdage[i] = make_int4(e.qcd[0], e.qage[0], e.qcd[1], e.qage[1]);
    a.v.misc[i] = make_int2(e.ticks, (int)f);
  } else {
    const uint32_t o16 = (uint32_t)i * 16u, o8 = (uint32_t)i * 8u;
    __builtin_amdgcn_raw_buffer_store_b128((skb4i){e.px[0], e.py[0], e.px[1], e.py[1]}, r, o16 + a.off[0], 0, 16);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(skb4i, (skb2d){e.rot[0], e.rot[1]}), r,
                                           o16 + a.off[1], 0, 16);
    __builtin_amdgcn_raw_buffer_store_b128((skb4i){e.qx[0], e.qy[0], e.qx[1], e.qy[1]}, r, o16 + a.off[2], 0, 16);
    if (qrot_changed)
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(skb4i, (skb2d){e.qrot[0], e.qrot[1]}), r,
                                             o16 + a.off[3], 0, 16);
    __builtin_amdgcn_raw_buffer_store_b128((skb4i){e.qcd[0], e.qage[0], e.qcd[1], e.qage[1]}, r, o16 + a.off[4], 0,
                                           16);
    __builtin_amdgcn_raw_buffer_store_b64((skb2i){e.ticks, (int)f}, r, o8 + a.off[5], 0, 16);
  }
}

// ---- the packed form (its range tests: sk_range.hpp, host-compilable)
using skrange::pack_fits_game;
using skrange::pack_fits_player;
__device__ __forceinline__ unsigned pack_flags(int qv0, int qv1, int live, int winner) {
  return (unsigned)qv0 | ((unsigned)qv1 << 1) | ((unsigned)live << 2) | ((unsigned)winner << 3);
}
__device__ __forceinline__ int pack_pos(int px, int py, int qx, int qy) {
  return (int)((unsigned)px | ((unsigned)py << 8) | ((unsigned)qx << 16) | ((unsigned)qy << 24));
}
__device__ __forceinline__ int pack_cah(int cd, int age, unsigned hi) {
  return (int)(((unsigned)cd & 0xffu) | ((unsigned)age << 8) | (hi << 16));
}

template <int POL>
__device__ __forceinline__ void store_env_pack(const MultiArgs& a, __amdgpu_buffer_rsrc_t rp, int64_t i, const Env& e,
                                               bool store_q) {
  const skb4i rb = __builtin_bit_cast(skb4i, (skb2d){e.rot[0], e.rot[1]});
  const skb4i qb = __builtin_bit_cast(skb4i, (skb2d){e.qrot[0], e.qrot[1]});
  const skb4i sb = {pack_pos(e.px[0], e.py[0], e.qx[0], e.qy[0]), pack_cah(e.qcd[0], e.qage[0], (unsigned)e.ticks),
                    pack_pos(e.px[1], e.py[1], e.qx[1], e.qy[1]),
                    pack_cah(e.qcd[1], e.qage[1], pack_flags(e.qvalid[0], e.qvalid[1], e.live, e.winner))};
  if constexpr (POL == 0) {
    skb4i* P = reinterpret_cast<skb4i*>(a.pack);
    P[i] = rb;
    if (store_q) P[a.n + i] = qb;
    P[2 * a.n + i] = sb;
  } else {
    const uint32_t o = (uint32_t)i * 16u, plane = (uint32_t)a.n * 16u;
    __builtin_amdgcn_raw_buffer_store_b128(rb, rp, o, 0, 16);
    if (store_q) __builtin_amdgcn_raw_buffer_store_b128(qb, rp, o + plane, 0, 16);
    __builtin_amdgcn_raw_buffer_store_b128(sb, rp, o + 2u * plane, 0, 16);
  }
}

struct MultiLane {
  int64_t i, ic;  // game; the game this lane loads (lanes past the end of a ragged batch: game 0, no stores)
  bool in, early;
  unsigned n_done, n_h1, n_h2, t_sum;  // this lane's episode counts (t_sum < n_ticks * tick_limit)
};

// one tick of k_step_multi.  The tick's own loads are its state; its action
// slab is already in registers (loaded a tick ahead) or in LDS (the feed
// wave), see k_step_multi.  Round 3's first prefetch of the next tick's slab
// (before the tick was split at its loads) was slower (65,536 games 2.51 vs
// 2.36 us per tick, 8,192 split 1.71 vs 1.59;
// profiles/r03d_multi_prefetch_sweep.jsonl): vector memory returns in issue
// order, so the next tick's state waited for the prefetched HBM loads anyway.
// `packed` (wave-uniform): where the state lives now; `last`: the final tick
// (its state goes to the exchange format).
//
// Round 5 (the K = 20 launch's fixed cost): the prologue
// had waited on six serial scalar rounds (kernel-argument lines as the
// scheduler reached them, the RNG step slot behind them) before its first
// state load; now every argument line comes in one round (the kernel's
// entry asm) and the step is formed only where a restart draws it
// (multi_step).  The tick is split at its loads (multi_load: the raw
// registers; multi_compute: decode and the rest).  Rotating the loop at
// those loads (tick t + 1's loads at the end of tick t's body, the counts
// summed in the last tick) measured slower (2.45-2.47 vs 2.38-2.42 us per
// tick at K = 4,000; profiles/r05b_multi_prologue_ab.jsonl), as did the same
// rotation in k_step_split_multi (8,192 games 1.68 vs 1.58 us), so the loop
// keeps its loads at the top.
struct MultiRaw {  // one tick's loads as issued, decoded at the tick's start
  skb4i v[5];       // pos, rot, qpos, qrot, qcdage (packed form: R, Q, S in v[0..2])
  skb2i m;          // misc
  float2 act[2];    // both players' actions
};

// the state loads of one tick (w.act is filled by k_step_multi: the slab
// loaded a tick ahead, or the feed wave's LDS slot).  `slab` is no longer
// read here; without the parameter the compiler orders k_step_multi's
// register copies at the loop's back edge differently, so it goes with the
// next change that is meant to alter the kernel.
template <int POL, bool PACK>
__device__ __forceinline__ void multi_load(const MultiArgs& a, __amdgpu_buffer_rsrc_t r, __amdgpu_buffer_rsrc_t rp,
                                           const MultiLane& L, int64_t slab, bool packed, MultiRaw& w) {
  const uint32_t o16 = (uint32_t)L.ic * 16u, o8 = (uint32_t)L.ic * 8u;
  if (PACK && packed) {
    if constexpr (POL == 0) {
      const skb4i* P = reinterpret_cast<const skb4i*>(a.pack);
      w.v[0] = P[L.ic];
      w.v[1] = P[a.n + L.ic];
      w.v[2] = P[2 * a.n + L.ic];
    } else {
      const uint32_t plane = (uint32_t)a.n * 16u;
      w.v[0] = __builtin_amdgcn_raw_buffer_load_b128(rp, o16, 0, 16);
      w.v[1] = __builtin_amdgcn_raw_buffer_load_b128(rp, o16 + plane, 0, 16);
      w.v[2] = __builtin_amdgcn_raw_buffer_load_b128(rp, o16 + 2u * plane, 0, 16);
    }
  } else if constexpr (POL == 0) {
    w.v[0] = __builtin_bit_cast(skb4i, a.v.pos[L.ic]);
    w.v[1] = __builtin_bit_cast(skb4i, a.v.rot[L.ic]);
    w.v[2] = __builtin_bit_cast(skb4i, a.v.qpos[L.ic]);
    w.v[3] = __builtin_bit_cast(skb4i, a.v.qrot[L.ic]);
    w.v[4] = __builtin_bit_cast(skb4i, a.v.qcdage[L.ic]);
    w.m = __builtin_bit_cast(skb2i, a.v.misc[L.ic]);
  } else {
#pragma unroll
    for (int k = 0; k < 5; ++k) w.v[k] = __builtin_amdgcn_raw_buffer_load_b128(r, o16 + a.off[k], 0, 16);
    w.m = __builtin_amdgcn_raw_buffer_load_b64(r, o8 + a.off[5], 0, 16);
  }
  __builtin_amdgcn_sched_barrier(0);
}

template <bool PACK>
__device__ __forceinline__ void multi_decode(const MultiRaw& w, bool packed, Env& e) {
  if (PACK && packed) {
    const skb2d rr = __builtin_bit_cast(skb2d, w.v[0]), qr = __builtin_bit_cast(skb2d, w.v[1]);
    e.rot[0] = rr.x; e.rot[1] = rr.y;
    e.qrot[0] = qr.x; e.qrot[1] = qr.y;
    const skb4i sb = w.v[2];
    const unsigned s0 = (unsigned)sb.x, c0 = (unsigned)sb.y, s1 = (unsigned)sb.z, c1 = (unsigned)sb.w;
    e.px[0] = s0 & 0xff; e.py[0] = (s0 >> 8) & 0xff; e.qx[0] = (s0 >> 16) & 0xff; e.qy[0] = s0 >> 24;
    e.px[1] = s1 & 0xff; e.py[1] = (s1 >> 8) & 0xff; e.qx[1] = (s1 >> 16) & 0xff; e.qy[1] = s1 >> 24;
    e.qcd[0] = (int)(signed char)(c0 & 0xff); e.qage[0] = (c0 >> 8) & 0xff;
    e.qcd[1] = (int)(signed char)(c1 & 0xff); e.qage[1] = (c1 >> 8) & 0xff;
    e.ticks = (int)(c0 >> 16);
    const unsigned fl = c1 >> 16;
    e.qvalid[0] = fl & 1; e.qvalid[1] = (fl >> 1) & 1; e.live = (fl >> 2) & 1; e.winner = (fl >> 3) & 3;
  } else {
    const skb4i p = w.v[0], q = w.v[2], ca = w.v[4];
    const skb2d rr = __builtin_bit_cast(skb2d, w.v[1]), qr = __builtin_bit_cast(skb2d, w.v[3]);
    decode_env(EnvRaw{make_int4(p.x, p.y, p.z, p.w), make_double2(rr.x, rr.y), make_int4(q.x, q.y, q.z, q.w),
                      make_double2(qr.x, qr.y), make_int4(ca.x, ca.y, ca.z, ca.w), make_int2(w.m.x, w.m.y)},
               e);
  }
}

// The RNG step of a tick, step0 + tick, formed only where a draw needs it:
// the empty asm keeps the sum (and the Philox products of it) from being
// hoisted to the loop's head, where the wait for the step slot's load would
// sit in front of every tick's compute.
__device__ __forceinline__ uint64_t multi_step(uint64_t step0, int tick) {
  asm volatile("" : "+v"(step0));
  return step0 + (uint64_t)tick;
}

// Measurement build only (-DSK_TRACE_MULTI; tools/trace_multi.py): lane 0 of
// every k_step_multi wave records s_memrealtime (100 MHz) at entry, after
// each of the first 29 ticks and at exit into sk_multi_trace[wave][32], and
// its hardware slot (HW_ID, XCC_ID) in word 30 (vector stores).
#if defined(SK_TRACE_MULTI_WAIT) && !defined(SK_TRACE_MULTI)
#define SK_TRACE_MULTI
#endif
#ifdef SK_TRACE_MULTI
__device__ unsigned long long* sk_multi_trace;
extern "C" int skdiag_set_multi_trace(void* buf) {
  return hipMemcpyToSymbol(HIP_SYMBOL(sk_multi_trace), &buf, sizeof(buf)) == hipSuccess ? 0 : -1;
}
#define SK_MTS(k)                                                                                   \
  do {                                                                                              \
    if ((threadIdx.x & 63) == 0)                                                                    \
      sk_multi_trace[((size_t)blockIdx.x * (blockDim.x == 128 ? 1 : blockDim.x / 64) + (threadIdx.x >> 6)) * 32 + (k)] = \
          __builtin_amdgcn_s_memrealtime();                                                         \
  } while (0)
#else
#define SK_MTS(k) \
  do {            \
  } while (0)
#endif

// SK_TRACE_MULTI_WAIT: ticks 0..4, five stamps each (loads issued, loads
// arrived, tick_env done, done / reset done, state stored)
#ifdef SK_TRACE_MULTI_WAIT
#define SK_MTW(tick, k) \
  do {                  \
    if ((tick) < 5) SK_MTS(1 + 5 * (tick) + (k)); \
  } while (0)
#else
#define SK_MTW(tick, k) \
  do {                  \
  } while (0)
#endif

// the rest of the tick on the loaded state; `last`: the launch's final tick
template <int POL, bool PACK>
__device__ __forceinline__ void multi_compute(const MultiArgs& a, const Cfg& c, __amdgpu_buffer_rsrc_t r,
                                              __amdgpu_buffer_rsrc_t rp, MultiLane& L, WaveCtr& wc, int64_t t,
                                              uint64_t step0, int tick, const MultiRaw& w, bool& packed,
                                              bool last, TrigCarry& tc) {
  Env e;
  multi_decode<PACK>(w, packed, e);
  const float2* acts = w.act;
  const double q_old0 = e.qrot[0], q_old1 = e.qrot[1];
  U4 ru = {0u, 0u, 0u, 0u};
  if (L.early) {  // the restart's draw under the loads (k_step)
    ru = draw4(a.seed, (uint64_t)(a.env_offset + L.i), multi_step(step0, tick), 1u);
    asm volatile("" : "+v"(ru.x), "+v"(ru.y), "+v"(ru.z), "+v"(ru.w));
  }
  __builtin_amdgcn_sched_barrier(0);
  // k_step's fp64 tick.  k_step_fast's (fp32 trig, exact fp64 redo) was no
  // faster at 400 ticks per launch and 20 % slower at 20 (65,536 games:
  // 2.50 vs 2.51 and 3.37 vs 2.71 us per tick; profiles/
  // r03i_multi_fast_early_sweep.jsonl).  Round 6: the same values with
  // the sincos carried from the previous tick (tick_env_carry, sk_device.hpp)
  tick_env_carry(c, e, tc, L.in, acts[0].x, acts[0].y, acts[1].x, acts[1].y);
  SK_MTW(tick, 2);
  // The state goes out right after the tick (early store),
  // before the done outputs and the restart; a lane that restarts stores its
  // planes again (its later stores win: same wave, same addresses, issue
  // order).  The stores then drain while the wave finishes the tick instead
  // of queueing in front of the next tick's loads (65,536 games: 2.22 -> 2.10
  // us per tick at 400 ticks per launch, 2.6 -> 2.5 at 20; profiles/r06n_*).
  // Storing pos / rot / qrot earlier still, between do_actions and game_tick,
  // was slower (2.02 -> 2.13, 2.54 -> 2.59; profiles/r06o_*).
  // The packed form stores early too (round 8; it had stored after the
  // restart): the pack decision is taken here, on the post-tick state (a
  // restart state always fits: the host checks the configuration's restart
  // positions).  114,688 games 3.00-3.03 vs 3.12-3.19 us per tick at 400
  // ticks per launch, 3.21-3.24 vs 3.42-3.48 at 20; 131,072 3.05-3.06 vs
  // 3.09-3.19; 262,144 5.17-5.40 vs 5.55-5.73 and 5.64-5.67 vs 6.00-6.15
  // (profiles/r08_lane_pack_early_ab.jsonl)
  bool to_pack = false;
  if constexpr (PACK) {
    const bool fit =
        !L.in || ((int)pack_fits_player(e.px[0], e.py[0], e.qx[0], e.qy[0], e.qcd[0], e.qage[0], e.qvalid[0]) &
                  (int)pack_fits_player(e.px[1], e.py[1], e.qx[1], e.qy[1], e.qcd[1], e.qage[1], e.qvalid[1]) &
                  (int)pack_fits_game(e.ticks, e.live, e.winner));
    to_pack = a.pack != nullptr && !last && __ballot(!fit) == 0;  // wave-uniform
  }
  if (L.in) {
    if (PACK && to_pack) {
      const bool qch = !packed || (__double_as_longlong(e.qrot[0]) != __double_as_longlong(q_old0)) ||
                       (__double_as_longlong(e.qrot[1]) != __double_as_longlong(q_old1));
      store_env_pack<POL>(a, rp, L.i, e, qch);
    } else {
      store_env_port<POL>(a, r, L.i, e, q_old0, q_old1, packed);
    }
  }
  // every load of this tick consumed (the counter slot's, issued first, with
  // them): without this the waitcnt pass, its tracking lost across the loop,
  // drains every store before the final counter store
  ctr_settle(wc);
  const bool d = L.in && ((!e.live) || (e.ticks >= a.tick_limit));  // SkillshotLearner.py:302
  if (L.in) {
    if (a.done) a.done[(int64_t)t * a.out_stride + L.i] = (uint8_t)d;
    if (a.winner) a.winner[(int64_t)t * a.out_stride + L.i] = (uint8_t)e.winner;
  }
  L.n_done += d;
  L.n_h1 += d && e.winner == 1;
  L.n_h2 += d && e.winner == 2;
  L.t_sum += d ? (unsigned)e.ticks : 0u;
  if (d && a.auto_reset) {
    if (a.random_positions) {
      if (L.early) reset_random_u(c, e, ru);
      else reset_random(c, e, a.seed, (uint64_t)(a.env_offset + L.i), multi_step(step0, tick));
    } else {
      reset_fixed(c, e);
    }
  }
  if (!last) carry_note(tc, e);
  SK_MTW(tick, 3);
  if (d && a.auto_reset) {  // the restarted game
    if (PACK && to_pack) store_env_pack<POL>(a, rp, L.i, e, true);
    else store_env_port<POL>(a, r, L.i, e, q_old0, q_old1, true);
  }
  packed = to_pack;
}


// PF > 0: one more wave per workgroup pulls the action slab PF ticks ahead
// into the CU's L1 / the XCD's L2 (global -> LDS copies into a scratch line
// nobody reads: no VGPR results to wait for), so the tick's own action loads
// hit cache instead of waiting for HBM.  The ring is larger than the
// Infinity Cache, so every slab is still fetched from HBM once; only the
// wait moves off the tick's dependency chain (the state loads cannot move:
// tick t + 1 reads what tick t stored).  The two waves meet at one raw
// s_barrier per tick, which keeps the prefetch PF ticks ahead and no more.
// the workgroup's GAMES games of both action planes, 16 bytes (two games of
// one plane) per lane and GAMES / 64 wave-instructions
template <int GAMES>
__device__ __forceinline__ void prefetch_slab(const MultiArgs& a, int64_t slab, int4* scratch) {
  static_assert(GAMES % 32 == 0, "whole 16-byte lines per plane");
  const int lane = threadIdx.x & 63;
  const int64_t g0 = (int64_t)blockIdx.x * GAMES;
#pragma unroll
  for (int j = 0; j < (GAMES + 63) / 64; ++j) {
    const int l = 64 * j + lane, pl = l / (GAMES / 2);
    const int64_t g = g0 + 2 * (l - pl * (GAMES / 2));
    if (l < GAMES && g + 1 < a.n)
      __builtin_amdgcn_global_load_lds((void*)(a.actions + (slab * 2 + pl) * a.n + g), scratch, 16, 0, 0);
  }
}

// the prefetch wave's loop (see k_step_multi): n_ticks raw barriers, slab of
// tick t + PF after the t-th
template <int GAMES, int PF>
__device__ __forceinline__ void prefetch_wave(const MultiArgs& a, int4* scratch) {
  int64_t s = a.slab0;  // the slab of tick t + PF (of tick 0 before the loop)
  for (int t = 0; t < a.n_ticks; ++t) {
    __builtin_amdgcn_s_barrier();
    if (t == 0) {  // ticks 1 .. PF - 1 (tick 0 loads its own slab; past n_ticks s is never used)
      for (int k = 1; k < PF && k < a.n_ticks; ++k) {
        s = s + 1 == a.ring ? 0 : s + 1;
        prefetch_slab<GAMES>(a, s, scratch);
      }
    }
    s = s + 1 == a.ring ? 0 : s + 1;
    if (t + PF < a.n_ticks) prefetch_slab<GAMES>(a, s, scratch);
  }
  __builtin_amdgcn_s_waitcnt(0);  // no LDS write outlives the workgroup
}

// k_step_multi's feed wave (PF > 0; round 6): the action slabs come to the
// stepping wave through LDS, not through its own vector-memory queue.  A
// tick's loads are consumed in issue order (vmcnt), so a tick that loads its
// slab waits for the slowest of its loads, the slab from HBM (the 400-slab
// ring is larger than the Infinity Cache), and any slab load issued earlier
// by the same wave is waited for by the next tick's state wait anyway.  A
// second wave of the workgroup copies the slab of tick t + PF into LDS slot
// (t + PF) % (PF + 1) (global -> LDS DMA, 16 B per lane: the workgroup's 64
// games of both planes in one wave-instruction), waits for the copy of tick
// t + 1 and meets the stepping wave at barrier t + 1; the stepping wave reads
// its two float2 from slot t % (PF + 1) after barrier t.  The slot a copy
// overwrites was read at tick t - 1, before the stepping wave reached barrier
// t.  Needs n % 64 == 0 (whole 16-byte pairs; the host checks).  The state's
// round trip is untouched: only the slab's HBM latency leaves the chain.
struct FeedSlot {
  float2 act[2][64];  // [plane][game of the workgroup]
};

__device__ __forceinline__ void feed_slab(const MultiArgs& a, int64_t slab, FeedSlot* dst) {
  const int lane = threadIdx.x & 63, pl = lane >> 5;
  const int64_t g = (int64_t)blockIdx.x * 64 + 2 * (lane & 31);
  __builtin_amdgcn_global_load_lds((void*)(a.actions + (slab * 2 + pl) * a.n + g), (void*)dst, 16, 0, 0);
}

// wait until at most n (0..3) of this wave's vector-memory operations are outstanding
__device__ __forceinline__ void wait_vm_upto(int n) {
  if (n >= 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
  else if (n == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  else if (n == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <int PF>
__device__ __forceinline__ void feed_wave(const MultiArgs& a, FeedSlot* slots) {
  static_assert(PF >= 1 && PF <= 4, "vmcnt immediates cover PF <= 4");
  constexpr int S = PF + 1;
  int64_t s = a.slab0;  // the next slab to copy
#pragma unroll
  for (int k = 0; k < PF; ++k) {  // ticks 0 .. PF - 1
    if (k < a.n_ticks) {
      feed_slab(a, s, slots + k);
      s = s + 1 == a.ring ? 0 : s + 1;
    }
  }
  int put = PF;  // slot of tick t + PF
  for (int t = 0; t < a.n_ticks; ++t) {
    // tick t's copy done: the copies issued after it (ticks t + 1 .. t + PF - 1) may fly
    const int younger = min(PF - 1, a.n_ticks - 1 - t);
    wait_vm_upto(younger);
    asm volatile("s_barrier" ::: "memory");  // barrier t: the stepping wave reads slot t % S
    if (t + PF < a.n_ticks) {
      feed_slab(a, s, slots + put);
      s = s + 1 == a.ring ? 0 : s + 1;
    }
    put = put + 1 == S ? 0 : put + 1;
  }
}

template <int POL, bool PACK, int BLK, int PF = 0>
__global__ void __launch_bounds__(BLK + (PF > 0 ? 64 : 0)) k_step_multi(MultiArgs a, Cfg c, int early) {
  static_assert(PF == 0 || BLK == 64, "the feed wave serves one 64-game wave");
  __shared__ FeedSlot feed[PF > 0 ? PF + 1 : 1];
  if constexpr (PF > 0) {
    if (threadIdx.x >= BLK) {  // the feed wave: n_ticks barriers, like the stepping wave
      feed_wave<PF>(a, feed);
      return;
    }
  }
  SK_MTS(0);
#ifdef SK_TRACE_MULTI  // slot 30: where the wave runs (HW_ID | XCC_ID << 32)
  if ((threadIdx.x & 63) == 0)
    sk_multi_trace[((size_t)blockIdx.x * (blockDim.x == 128 ? 1 : blockDim.x / 64) + (threadIdx.x >> 6)) * 32 + 30] =
        (unsigned long long)__builtin_amdgcn_s_getreg(4 | (31 << 11)) |
        ((unsigned long long)__builtin_amdgcn_s_getreg(20 | (31 << 11)) << 32);
#endif
  // every kernel-argument line the launch reads, fetched in ONE scalar round
  // before anything else (the empty asm consumes a word of each 64-B line of
  // MultiArgs; left to the scheduler, the lines came in three dependent rounds
  // around tick 0's loads)
  asm volatile("" ::"s"(a.n), "s"(a.out_stride), "s"(a.off[0]), "s"(a.off[5]), "s"(c.cdmax), "s"(early));
  MultiLane L;
  L.i = (int64_t)blockIdx.x * BLK + threadIdx.x;
  L.in = L.i < a.n;
  L.ic = L.in ? L.i : 0;
  L.early = a.random_positions && early;
  L.n_done = L.n_h1 = L.n_h2 = L.t_sum = 0;
  const __amdgpu_buffer_rsrc_t r = raw_rsrc(a.base), rp = raw_rsrc(a.pack);
  int64_t slab = a.slab0, so = a.out0;
  bool packed = false;  // every launch starts from (and ends in) the exchange format
  // the counter slot and the RNG step slot load first (their values are
  // needed at the launch's end, or only on a restart: multi_step), the step
  // slot's advance at the launch's end (it had been a store in the prologue)
  WaveCtr wc = ctr_load<BLK>(a.ctr);
  const uint64_t step0 = step_read(a.step);
  int t = 0;
  TrigCarry tc;
  tc.have = tc.pend = false;
  // The action pipeline (no feed wave): a tick's action slab is loaded one
  // tick before it, into registers, after that earlier tick's state loads.
  // The 400-slab ring is larger than the Infinity Cache, so a slab comes from
  // HBM, later than the state from the fabric; a tick's loads are consumed in
  // issue order (vmcnt), so with the slab among them its wait was the slab's
  // HBM latency (65,536 games, 20-tick launches: 2.55 us per tick with the
  // HBM ring against 2.04 with an 8-slab ring held in cache;
  // profiles/r06f_multi_pack_pf_ring_sweep.jsonl).  Issued one tick ahead, the
  // slab's loads are older than the state loads its tick waits for by a whole
  // tick; more ticks ahead gain nothing, since tick t + 1 waits (in issue
  // order) for every load tick t issued.  Tick t reads the slab from one
  // register pair while the next tick's slab loads into the other; the loop
  // runs two ticks per iteration so the pairs alternate without a copy (a
  // copy of the pair just loaded waits for that load)
  constexpr bool AHEAD = PF == 0;
  float2 pa0[2], pa1[2];
  if constexpr (AHEAD) {
    pa0[0] = load_action(a.actions + slab * 2 * a.n + L.ic);
    pa0[1] = load_action(a.actions + slab * 2 * a.n + a.n + L.ic);
  }
  int64_t pslab = slab + 1 == a.ring ? 0 : slab + 1;  // the slab of tick t + 1
  int take = 0;  // the feed slot of tick t
  auto one_tick = [&](float2 (&cur)[2], float2 (&nxt)[2]) {
    MultiRaw w;
    if constexpr (PF > 0) asm volatile("s_barrier" ::: "memory");  // barrier t (feed_wave)
    multi_load<POL, PACK>(a, r, rp, L, slab, packed, w);  // the state; the slab comes from LDS or from `cur`
    if constexpr (PF > 0) {  // the slab from LDS (feed_wave)
      const int gl = threadIdx.x & 63;
      w.act[0] = feed[take].act[0][gl];
      w.act[1] = feed[take].act[1][gl];
      take = take == PF ? 0 : take + 1;
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (AHEAD) {
      // after this tick's state loads, unconditionally (a load under a
      // branch made the waitcnt pass drain every load before the compute);
      // past the launch's last tick it re-reads this tick's slab
      const int64_t ls = t + 1 < a.n_ticks ? pslab : slab;
      nxt[0] = load_action(a.actions + ls * 2 * a.n + L.ic);
      nxt[1] = load_action(a.actions + ls * 2 * a.n + a.n + L.ic);
      w.act[0] = cur[0];
      w.act[1] = cur[1];
      __builtin_amdgcn_sched_barrier(0);
    }
    if (tc.pend) carry_advance(tc);  // the last tick's rotations, while this tick's loads fly
    __builtin_amdgcn_sched_barrier(0);
#ifdef SK_TRACE_MULTI_WAIT
    if (t < 5) {
      SK_MTW(t, 0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      SK_MTW(t, 1);
    }
#endif
    multi_compute<POL, PACK>(a, c, r, rp, L, wc, so, step0, t, w, packed, t + 1 == a.n_ticks, tc);
#if defined(SK_TRACE_MULTI_WAIT)
    SK_MTW(t, 4);
#elif defined(SK_TRACE_MULTI)
    if (t < 29) SK_MTS(1 + t);
#endif
    slab = slab + 1 == a.ring ? 0 : slab + 1;
    pslab = pslab + 1 == a.ring ? 0 : pslab + 1;
    so = so + 1 == a.out_slabs ? 0 : so + 1;
  };
  do {  // n_ticks >= 1 (host-checked): every path to the counter store passes ctr_settle
    one_tick(pa0, pa1);
    if (++t >= a.n_ticks) break;
    one_tick(pa1, pa0);
  } while (++t < a.n_ticks);
  if (a.ctr) {
    const unsigned c4[4] = {L.n_done, L.n_h1, L.n_h2, L.t_sum};
    uint64_t v[4];
    wave_sum4_u32(c4, v);
    ctr_store<BLK>(a.ctr, wc, v[0], v[1], v[2], v[3]);
  }
  step_advance(a.step, step0, (uint64_t)a.n_ticks);
  SK_MTS(31);
}

// k_step_split_multi: k_step_multi with k_step_split's geometry — lanes (2i,
// 2i+1) own players 1 and 2 of game i, each loading and storing its player's
// 8-byte half of every plane (the pair covers the game's 16 bytes; a wave
// moves 512 contiguous bytes per plane), exchanging positions / projectiles
// with pair_swap (DPP) for the collision test.  Twice the waves of
// k_step_multi at half the dependent chain per lane: at 65,536 games two
// waves share each SIMD, so one wave's state round trip through memory
// overlaps the other's tick.  Same contract, same state ports.  The packed
// form is a compile-time instantiation (PACK), chosen by the host for
// kSplitPackMinEnvs .. kSplitPackMaxEnvs games: as a runtime branch it cost
// the small grids a quarter of their tick (8,192 games 1.98 vs 1.59 us;
// profiles/r03f_multi_pack*_sweep.jsonl vs r03c_multi_split_sweep.jsonl).
template <int POL>
__device__ __forceinline__ void st_half_d(const MultiArgs& a, __amdgpu_buffer_rsrc_t r, int k, double* plane, int64_t h,
                                          double v) {
  if constexpr (POL == 0) plane[h] = v;
  else __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(skb2i, v), r, (uint32_t)h * 8u + a.off[k], 0, 16);
}
template <int POL>
__device__ __forceinline__ void st_half_i(const MultiArgs& a, __amdgpu_buffer_rsrc_t r, int k, int2* plane, int64_t h,
                                          int x, int y) {
  if constexpr (POL == 0) plane[h] = make_int2(x, y);
  else __builtin_amdgcn_raw_buffer_store_b64((skb2i){x, y}, r, (uint32_t)h * 8u + a.off[k], 0, 16);
}
struct SplitLane {
  int64_t i, ic, hc, h;  // game, loaded game, loaded / stored half-plane index
  int p;                 // player of this lane
  bool in;
  unsigned n_done, n_h1, n_h2, t_sum;  // this pair's episode counts (lane p = 0 counts)
};

// ---- the split tick (split_tick_carry): k_step_multi's carried-sincos tick
// in the split geometry.  The lane's player's rotation sincos is
// carried from the previous tick (evaluated at the top of the tick after its
// loads are issued, keyed by the rotation's bits), a projectile in flight keeps its
// carried sincos, a fired one gets its step by fp32 angle addition with the
// wave's exact fallback (tick_env_carry, sk_device.hpp); the commits are
// selects; the action slab is loaded one tick ahead; the state halves are
// stored right after the tick, before done / restart (a restarted game's
// lanes store theirs again).  Bit for bit k_step_split launched once per tick
// (tests/test_multi_gpu.py and tests/test_multi_obs_gpu.py compare a launch
// with one sk_env_step launch per tick).
struct SplitCarry {
  double kr, kq;  // keys: m = sincos(kr), tq = sincos(kq)
  sktrig::SinCos m, tq;
  double pr;      // the last tick's final rotation (evaluated at the next tick's top)
  bool qs, have, pend;
};
__device__ __forceinline__ void split_carry_advance(SplitCarry& t) {
  bool k;
  t.m = sktrig::sincos_bf(t.pr, &k);
  if (!k) t.m = sincos_lib(t.pr);
  t.kr = t.pr;
  if (t.qs) {
    t.tq = t.m;
    t.kq = t.pr;
  }
  t.have = true;
  t.pend = false;
}
// FAST (step-only): the carry in fp32.  The tick never stores a sine, only
// int(round(p - d)), so what is carried is sincos_fast of the rotation (the
// move's deltas and a fired projectile's angle addition start from it) and,
// for the projectile in flight, its integer step: round_safe holds for every
// integer p, so the step rintf(ex), rintf(ey) taken at the launch is the
// flight's.  `qex`: that step could not be decided in fp32 (a delta within
// its bound of a half-integer, or a rotation outside the fast range); such a
// lane sends its wave through the exact evaluation every tick of the flight.
struct SplitCarryF {
  double kr, kq;      // keys: m = sincos_fast(kr), (dx, dy) = the step of a projectile with rotation kq
  sktrig::SinCosF m;
  int dx, dy;
  double pr;          // the last tick's final rotation (evaluated at the next tick's top)
  bool mok, qex, have, pend;
};
__device__ __forceinline__ void split_carry_advance(SplitCarryF& t) {
  t.m = sktrig::sincos_fast(t.pr, &t.mok);
  t.kr = t.pr;
  t.have = true;
  t.pend = false;
}
// The advanced carry pinned where it stands (empty asms).  The steady loop
// advances unconditionally, and without this the evaluation is sunk past the
// loads' wait into the tick's no-miss branch, onto the chain it was taken off
// (the generic tick's `if (tc.pend)` block keeps it in place by itself).
__device__ __forceinline__ void split_carry_pin(SplitCarry& t) {
  asm volatile("" : "+v"(t.m.s), "+v"(t.m.c), "+v"(t.tq.s), "+v"(t.tq.c));
}
__device__ __forceinline__ void split_carry_pin(SplitCarryF& t) {
  asm volatile("" : "+v"(t.m.s), "+v"(t.m.c));
}
template <bool FAST>
struct SplitCarrySel {
  using type = SplitCarry;
};
template <>
struct SplitCarrySel<true> {
  using type = SplitCarryF;
};
struct SplitRaw {
  skb2i rot, qrot, pp, ca, qq, mi;
};
template <int POL>
__device__ __forceinline__ skb2i ld_half_raw(const MultiArgs& a, __amdgpu_buffer_rsrc_t r, int k, const void* plane,
                                             int64_t h) {
  if constexpr (POL == 0) return reinterpret_cast<const skb2i*>(plane)[h];
  else return __builtin_amdgcn_raw_buffer_load_b64(r, (uint32_t)h * 8u + a.off[k], 0, 16);
}
template <int POL>
__device__ __forceinline__ void split_load_raw(const MultiArgs& a, __amdgpu_buffer_rsrc_t r, const SplitLane& L,
                                               SplitRaw& w) {
  // k_step_split's load order: rotation first
  w.rot = ld_half_raw<POL>(a, r, 1, a.v.rot, L.hc);
  w.qrot = ld_half_raw<POL>(a, r, 3, a.v.qrot, L.hc);
  w.pp = ld_half_raw<POL>(a, r, 0, a.v.pos, L.hc);
  w.ca = ld_half_raw<POL>(a, r, 4, a.v.qcdage, L.hc);
  w.qq = ld_half_raw<POL>(a, r, 2, a.v.qpos, L.hc);
  w.mi = ld_half_raw<POL>(a, r, 5, a.v.misc, L.ic);
  __builtin_amdgcn_sched_barrier(0);
}
template <int POL>
__device__ __forceinline__ void split_store_state(const MultiArgs& a, __amdgpu_buffer_rsrc_t r, const SplitLane& L,
                                                  int px, int py, double rot, int qx, int qy, double qrot, bool qch,
                                                  int qcd, int qage, int ticks, unsigned f) {
  st_half_i<POL>(a, r, 0, reinterpret_cast<int2*>(a.v.pos), L.h, px, py);
  st_half_d<POL>(a, r, 1, reinterpret_cast<double*>(a.v.rot), L.h, rot);
  st_half_i<POL>(a, r, 2, reinterpret_cast<int2*>(a.v.qpos), L.h, qx, qy);
  if (qch) st_half_d<POL>(a, r, 3, reinterpret_cast<double*>(a.v.qrot), L.h, qrot);
  st_half_i<POL>(a, r, 4, reinterpret_cast<int2*>(a.v.qcdage), L.h, qcd, qage);
  if (L.p == 0) st_half_i<POL>(a, r, 5, a.v.misc, L.i, ticks, (int)f);
}
// The packed form in the split geometry (store_env_pack's layout: R double2[n],
// Q double2[n], S int4[n]): lane 2i + p owns player p's 8-byte half of each
// plane, the rotation, the projectile rotation and {pack_pos, pack_cah}.  The
// high half of player 1's cah word is the game's ticks, of player 2's its
// flag byte; the pair exchanges them with one pair_swap.  rp: the resource
// over a.pack (POL 1).
template <int POL>
__device__ __forceinline__ void split_load_pack(const MultiArgs& a, __amdgpu_buffer_rsrc_t rp, const SplitLane& L,
                                                SplitRaw& w) {
  if constexpr (POL == 0) {
    const skb2i* P = reinterpret_cast<const skb2i*>(a.pack);
    w.rot = P[L.hc];
    w.qrot = P[2 * a.n + L.hc];
    w.pp = P[4 * a.n + L.hc];
  } else {
    const uint32_t o = (uint32_t)L.hc * 8u, plane = (uint32_t)a.n * 16u;
    w.rot = __builtin_amdgcn_raw_buffer_load_b64(rp, o, 0, 16);
    w.qrot = __builtin_amdgcn_raw_buffer_load_b64(rp, o + plane, 0, 16);
    w.pp = __builtin_amdgcn_raw_buffer_load_b64(rp, o + 2u * plane, 0, 16);
  }
  // w.ca / qq / mi stay unwritten: a packed tick never reads them, and they
  // are the 88-B path's load destinations (writing them here made the wave
  // wait for its earlier stores before the work under the round trip began)
  __builtin_amdgcn_sched_barrier(0);
}
template <int POL>
__device__ __forceinline__ void split_store_pack(const MultiArgs& a, __amdgpu_buffer_rsrc_t rp, const SplitLane& L,
                                                 double rot, double qrot, bool store_q, int pos, int cah) {
  if constexpr (POL == 0) {
    skb2i* P = reinterpret_cast<skb2i*>(a.pack);
    P[L.h] = __builtin_bit_cast(skb2i, rot);
    if (store_q) P[2 * a.n + L.h] = __builtin_bit_cast(skb2i, qrot);
    P[4 * a.n + L.h] = (skb2i){pos, cah};
  } else {
    const uint32_t o = (uint32_t)L.h * 8u, plane = (uint32_t)a.n * 16u;
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(skb2i, rot), rp, o, 0, 16);
    if (store_q) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(skb2i, qrot), rp, o + plane, 0, 16);
    __builtin_amdgcn_raw_buffer_store_b64((skb2i){pos, cah}, rp, o + 2u * plane, 0, 16);
  }
}
// ... the {pack_pos, pack_cah} word alone (the steady tick's corrected flags)
template <int POL>
__device__ __forceinline__ void split_store_pack_word(const MultiArgs& a, __amdgpu_buffer_rsrc_t rp,
                                                      const SplitLane& L, int pos, int cah) {
  if constexpr (POL == 0) {
    reinterpret_cast<skb2i*>(a.pack)[4 * a.n + L.h] = (skb2i){pos, cah};
  } else {
    const uint32_t o = (uint32_t)L.h * 8u, plane = (uint32_t)a.n * 16u;
    __builtin_amdgcn_raw_buffer_store_b64((skb2i){pos, cah}, rp, o + 2u * plane, 0, 16);
  }
}
// OBS (the full contract, sk_env_step_multi_obs): the tick also evaluates
// the exact sincos of the post-look rotation (the obs epilogue's projectile
// sincos when it fires, and the next tick's carried move sincos: no
// evaluation at the next tick's top) and the fp32 one (obs12_sc's `pr`), and
// writes the observation and reward after the state stores.
//
// PACK (step-only): between the ticks of a launch the state lives in the
// packed 48-B form (split_load_pack / split_store_pack) while every lane of
// the wave fits it, as in multi_compute: `packed` (wave-uniform) says where
// this tick's state is and is set for the next tick.  The decision is taken
// on the post-tick state, before the early store (a restart state always
// fits: the host checks the configuration's restart positions); the
// launch's first tick loads and its last stores the exchange format, and a
// tick that follows a packed one stores the qrot plane regardless.
//
// FAST (step-only): fp32 trig off the carry with the wave's exact fallback
// (SplitCarryF; tick_env_fast's error budget).  The move's deltas come from
// the carried sincos_fast, a fired projectile's step from its angle addition,
// the step of one in flight is carried as two integers.  A wave with a lane
// whose move or fired step is within its bound of a half-integer, whose
// projectile in flight is flagged exact-only, whose rotation is outside the
// fast range or whose action is not finite evaluates sincos_bf (the library
// past its range) and takes the fp64 expressions of the other form: the same
// result bit for bit, about one wave-tick in a few hundred.
//
// STEADY (PACK only): the tick of the packed kernel's steady loop
// (k_step_split_multi).  Known at compile time: the state arrives packed,
// the tick is not the launch's last, the carry is valid, and the state leaves
// packed: the generic tick admitted the wave for the rest of the launch
// (skrange::admit_*: no state of it can stop fitting), so the steady tick has
// no fit test and no exchange-format stores.  The done / winner rows go
// through buffer resources at 32-bit offsets (SplitSteady), and the episode
// counts and the restart sit behind one ballot of `done`: a wave of 32 games
// has a finished one in about one tick in forty.  Its range tests (the
// move's and the projectile's bounds, the collision's intervals) take one
// unsigned compare each (sk_range.hpp; the host admits a launch to the steady
// loop only for a configuration where that form is exact, skrange::cfg_ok).
// The steady tick stores its state ahead of the collision test, as if nobody
// were hit: once the move, the fire, the projectile step and the clock are
// settled it exchanges the partner's `qvalid` and stores the three planes with
// `live` and `winner` as loaded; the exchanges of qx / qy, box_hit, the bit's
// exchange and pair_hit follow in the tail, where the wave rests anyway
// (kSteadyRest).  A hit makes the game `done`: inside the `any_done` block a
// game hit in this tick that does not restart stores its {pos, cah} word
// again (a restarting one all three planes, as before), after the first store
// in program order, from the same lane to the same address.  The FAST steady
// tick decides the exactness guard under its loads: `maybe`, the lanes with
// !msafe || !qsafe || qex, all known before the state arrives (SplitPre, the
// carry), is a superset of `un` lane by lane, so behind the wait a wave-tick
// where `maybe` is empty (all but about one in two hundred) takes one scalar
// branch, and only the others evaluate `un` and its ballot.  From the state
// wait to the last state store the full-wave tick has 102 instructions on its
// common path for 113 (profiles/r20_listing.txt), and that stretch runs at
// issue priority 1 (kSteadyPrio).
//
// FULL (STEADY only): every lane of the wave is in range, `L.in` is true at
// compile time: no lane mask around the key check, the stores
// and the done rows.  Every wave of a launch but at most its last.
//
// The PACK forms evaluate one collision test per lane, "my player is hit by
// the partner's projectile", and exchange the bit with one more pair_swap
// (65,536 games 1.53-1.55 against 1.59-1.60 us per tick; with the one-compare
// tests 1.46-1.49, with FULL 1.43-1.46; profiles/r13_bench_ab.jsonl).
struct SplitSteady {
  __amdgpu_buffer_rsrc_t ra, rd, rw;  // the action ring, done, winner (a NULL output: no records, its stores are dropped)
  uint32_t va, vd;                    // this lane's byte offset in an action slab / an output row
  uint32_t aso, dso;                  // the next tick's slab and this tick's output row, in bytes (wave-uniform)
  unsigned long long maybe;           // FAST: the lanes that may need the exact evaluation this tick (split_pre_maybe)
};
// The part of the FAST tick that reads no loaded state, only the carried
// sincos_fast of the rotation, the action and the configuration: the clamped
// look action and its rotation step, the fired projectile's angle addition
// and step, the move's deltas, their round_safe decisions and the rounded
// integers.  The steady loop evaluates it under its loads (split_pre_pin
// keeps it there, as split_carry_pin the carry); the tick combines the fired
// step's safety with `f` after the wait.  The same expressions on the same
// inputs as the generic tick's, so the same bits.
struct SplitPre {
  float l;            // the clamped look action
  double dl;          // (double)l * look: the rotation's step
  sktrig::SinCosF u;  // sincos_fast(rotation + l * look) by angle addition
  float ex, ey;       // a fired projectile's step
  float mdx, mdy;     // the move's deltas
  bool msafe, qsafe;  // fast_move_delta's / the fired step's `safe`
  int imx, imy, iex, iey;  // rintf of the deltas and of the step
};
__device__ __forceinline__ SplitPre split_fast_pre(const sktrig::SinCosF& m, bool mok, float2 act, const Cfg& c) {
  SplitPre q;
  const float qsf = (float)c.qspeed;
  q.l = clamp_action_f(act.y);
  q.dl = (double)q.l * c.look;
  q.u = sktrig::sincos_add(m, q.l * (float)c.look);
  q.ex = q.u.s * qsf;
  q.ey = q.u.c * qsf;
  const sktrig::FastDelta dm = sktrig::fast_move_delta(m, mok, (float)c.pspeed, clamp_action_f(act.x));
  q.mdx = dm.x;
  q.mdy = dm.y;
  q.msafe = dm.safe;
  q.qsafe = sktrig::fast_step_delta(q.u, mok, qsf).safe;  // its deltas are ex, ey
  q.imx = (int)rintf(q.mdx);
  q.imy = (int)rintf(q.mdy);
  q.iex = (int)rintf(q.ex);
  q.iey = (int)rintf(q.ey);
  return q;
}
// (the two decisions are pinned as the lane masks they are: every lane of the
// wave is active where the steady loop evaluates them; returns the lanes with
// a decision that is not safe, off the pinned masks: split_pre_unsafe)
__device__ __forceinline__ unsigned long long split_pre_pin(SplitPre& q) {
  unsigned long long ms = __builtin_amdgcn_ballot_w64(q.msafe), qs = __builtin_amdgcn_ballot_w64(q.qsafe);
  asm volatile("" : "+v"(q.dl), "+v"(q.imx), "+v"(q.imy), "+v"(q.iex), "+v"(q.iey), "+s"(ms), "+s"(qs));
  q.msafe = __builtin_amdgcn_inverse_ballot_w64(ms);
  q.qsafe = __builtin_amdgcn_inverse_ballot_w64(qs);
  return ~(ms & qs);
}
// The lanes whose tick may need the exact evaluation, from what is known
// before the state arrives: `un` of the tick is !msafe || (f && !qsafe) ||
// (qvalid && !f && qex), so lane by lane un implies !msafe || !qsafe || qex,
// whatever f and qvalid turn out to be.  `unsafe`: the lanes with !msafe ||
// !qsafe; `in`: the lanes in range.  An SGPR pair, nonzero in 0.48 % of the
// benchmark's wave-ticks.
__device__ __forceinline__ unsigned long long split_pre_maybe(unsigned long long unsafe, bool qex,
                                                              unsigned long long in) {
  unsigned long long m = (unsafe | __builtin_amdgcn_ballot_w64(qex)) & in;
  asm volatile("" : "+s"(m));
  return m;
}
// ... the lanes with a decision of `q` that is not safe (the key-miss block's refreshed SplitPre)
__device__ __forceinline__ unsigned long long split_pre_unsafe(const SplitPre& q) {
  return ~(__builtin_amdgcn_ballot_w64(q.msafe) & __builtin_amdgcn_ballot_w64(q.qsafe));
}
template <int POL, bool OBS, bool PACK = false, bool FAST = false, bool STEADY = false, bool FULL = false>
__device__ __forceinline__ void split_tick_carry(const MultiArgs& a, const Cfg& c, __amdgpu_buffer_rsrc_t r,
                                                 SplitLane& L, WaveCtr& wc, int64_t so, uint64_t step,
                                                 const SplitRaw& w, float2 act,
                                                 typename SplitCarrySel<FAST>::type& tc, bool last,
                                                 __amdgpu_buffer_rsrc_t rp, bool& packed,
                                                 SplitSteady* ss = nullptr, SplitPre* pre = nullptr,
                                                 int left = 0, bool* admit = nullptr) {
  constexpr bool PRE = FAST && STEADY;  // the state-independent part arrives evaluated (SplitPre)
  static_assert(!(OBS && PACK), "the full contract never packs");
  static_assert(!(OBS && FAST), "the observation needs the exact sincos");
  static_assert(PACK || !STEADY, "the steady loop is the packed kernel's");
  static_assert(STEADY || !FULL, "the full-wave form is the steady loop's");
  using sktrig::round_safe;
  const int p = L.p;
  const bool in = FULL || L.in;
  double rot = __builtin_bit_cast(double, w.rot), qrot = __builtin_bit_cast(double, w.qrot);
  int px = w.pp.x, py = w.pp.y, qx = w.qq.x, qy = w.qq.y, qcd = w.ca.x, qage = w.ca.y, ticks = w.mi.x;
  const unsigned flags = (unsigned)w.mi.y;
  int qvalid = (flags >> (8 * p)) & 0xff, live = (flags >> 16) & 0xff, winner = (flags >> 24) & 0xff;
  if constexpr (PACK) {
    if (STEADY || packed) {  // w.pp: {pack_pos, pack_cah} of this lane's player
      const unsigned s = (unsigned)w.pp.x, ch = (unsigned)w.pp.y;
      px = s & 0xff; py = (s >> 8) & 0xff; qx = (s >> 16) & 0xff; qy = s >> 24;
      qcd = (int)(signed char)(ch & 0xff); qage = (ch >> 8) & 0xff;
      const unsigned hi = ch >> 16, ohi = (unsigned)pair_swap((int)hi);
      const unsigned fl = p ? hi : ohi;
      ticks = (int)(p ? ohi : hi);
      qvalid = (fl >> p) & 1; live = (fl >> 2) & 1; winner = (fl >> 3) & 3;
    }
  }
  const double q_old = qrot;
  const bool f = qcd <= 0;  // fires this tick (Player.py:80)
  const bool miss = (!STEADY && !tc.have) || !same_bits(rot, tc.kr) || (qvalid && !f && !same_bits(qrot, tc.kq));
  if (__ballot(in && miss) != 0) {  // the launch's first tick
    if constexpr (FAST) {
      bool kq;
      tc.m = sktrig::sincos_fast(rot, &tc.mok);
      const sktrig::SinCosF q = sktrig::sincos_fast(qrot, &kq);
      const sktrig::FastDelta d = sktrig::fast_step_delta(q, kq, (float)c.qspeed);
      tc.qex = !d.safe;
      tc.dx = (int)rintf(d.x);
      tc.dy = (int)rintf(d.y);
    } else {
      bool k0, k1;
      tc.m = sktrig::sincos_bf(rot, &k0);
      tc.tq = sktrig::sincos_bf(qrot, &k1);
      if (!(k0 & k1)) {
        if (!k0) tc.m = sincos_lib(rot);
        if (!k1) tc.tq = sincos_lib(qrot);
      }
    }
    tc.kr = rot;
    tc.kq = qrot;
    tc.have = true;
    if constexpr (PRE) {  // off the refreshed carry
      *pre = split_fast_pre(tc.m, tc.mok, act, c);
      ss->maybe = split_pre_maybe(split_pre_unsafe(*pre), tc.qex, FULL ? ~0ull : __builtin_amdgcn_ballot_w64(in));
    }
  }
  SplitPre q{};
  if constexpr (PRE) q = *pre;
  const float l = PRE ? q.l : clamp_action_f(act.y);
  const double rn = rot + (PRE ? q.dl : (double)l * c.look);  // == move_look_s
  const float lk = (float)c.look, qsf = (float)c.qspeed, eq = 2e-6f * qsf;
  sktrig::SinCosF mf;
  if constexpr (FAST) mf = tc.m;
  else mf = sktrig::SinCosF{(float)tc.m.s, (float)tc.m.c};
  const sktrig::SinCosF u = PRE ? q.u : sktrig::sincos_add(mf, l * lk);
  const float ex = PRE ? q.ex : u.s * qsf, ey = PRE ? q.ey : u.c * qsf;
  bool un, unq = false;
  float mdx = 0.0f, mdy = 0.0f;  // FAST: the move's deltas
  sktrig::SinCos tt{0.0, 1.0};   // the projectile's exact sincos (FAST: on the exact path only)
  sktrig::SinCos tm{0.0, 1.0};   // the move's
  if constexpr (PRE) {
    mdx = q.mdx;
    mdy = q.mdy;
    unq = (int)f & (int)!q.qsafe;
    un = false;  // (decided below, and only in a wave-tick where some lane may: ss->maybe)
  } else if constexpr (FAST) {
    const sktrig::FastDelta dm = sktrig::fast_move_delta(tc.m, tc.mok, (float)c.pspeed, clamp_action_f(act.x));
    mdx = dm.x;
    mdy = dm.y;
    unq = f && !sktrig::fast_step_delta(u, tc.mok, qsf).safe;  // its deltas are ex, ey
    un = !dm.safe || unq || (qvalid && !f && tc.qex);
  } else {
    un = f && !((int)(fabs(rot) < c.fast_rot_max) & (int)round_safe(ex, eq) & (int)round_safe(ey, eq));
    tt = tc.tq;  // in flight: the carried exact value
    tm = tc.m;
  }
  bool fast = f;   // the fired step from fp32 (the other form)
  bool exact = false;  // FAST, wave-uniform: this tick takes the fp64 expressions' results
  int epx = 0, epy = 0, enx = 0, eny = 0;  // ... the post-move position and the projectile's candidate
  sktrig::SinCos xn{0.0, 1.0};    // OBS: sincos(rn), exact
  sktrig::SinCosF pr{0.0f, 1.0f};  // OBS: sincos(rn) in fp32 (obs12_sc)
  if constexpr (OBS) {
    bool kx, k2;
    xn = sktrig::sincos_bf(rn, &kx);
    pr = sktrig::sincos_fast(rn, &k2);
    if (!(kx & k2)) {
      if (!kx) xn = sincos_lib(rn);
      if (!k2) {
        const sktrig::SinCos rr = sincos_lib(rn);
        pr.s = (float)rr.s;
        pr.c = (float)rr.c;
      }
    }
  }
  bool any_un;  // wave-uniform
  if constexpr (PRE) {
    // un is a subset of ss->maybe lane by lane (split_pre_maybe), so a wave-tick
    // where nothing may takes one scalar branch here, no mask arithmetic
    any_un = false;
    if (__builtin_expect(ss->maybe != 0, 0)) {
      un = (int)!q.msafe | (int)unq | ((int)(qvalid != 0) & (int)!f & (int)tc.qex);
      any_un = __ballot(in && un) != 0;
    }
  } else {
    any_un = __ballot(in && un) != 0;
  }
  if (__builtin_expect(any_un, 0)) {  // the exact sincos of the fired projectiles
    if constexpr (FAST) {  // ... and of the move and the projectile in flight
      const double qa = f ? rn : qrot;
      bool k0, k1;
      tm = sktrig::sincos_bf(rot, &k0);
      tt = sktrig::sincos_bf(qa, &k1);
      if (!(k0 & k1)) {
        if (!k0) tm = sincos_lib(rot);
        if (!k1) tt = sincos_lib(qa);
      }
      // today's fp64 expressions of the other form, for the whole wave (a
      // lane the fast path could decide gets the same integers): the move,
      // then the projectile from where shoot leaves it
      const double speed = clamp_action((double)act.x), psp = (double)c.pspeed, qsp = (double)c.qspeed;
      const double nxf = __builtin_rint((double)px - (tm.s * psp) * speed);
      const double nyf = __builtin_rint((double)py - (tm.c * psp) * speed);
      const bool ok = (nxf >= 0.0) & (nxf + (double)c.psize <= (double)c.W) & (nyf >= 0.0) &
                      (nyf + (double)c.psize <= (double)c.H);
      epx = ok ? (int)(ok ? nxf : 0.0) : px;
      epy = ok ? (int)(ok ? nyf : 0.0) : py;
      enx = (int)__builtin_rint((double)(f ? epx : qx) - tt.s * qsp);
      eny = (int)__builtin_rint((double)(f ? epy : qy) - tt.c * qsp);
      exact = true;
    } else {
      sktrig::SinCos x = xn;
      if constexpr (!OBS) {
        bool k;
        x = sktrig::sincos_bf(rn, &k);
        if (!k) x = sincos_lib(rn);
      }
      if (f) tt = x;
      fast = false;
    }
  }
  sktrig::SinCos tq_obs{0.0, 1.0};  // OBS: the projectile's sincos after shoot
  if constexpr (OBS) tq_obs = f ? xn : tc.tq;
  // do_actions(p + 1, ...)  SkillshotLearner.py:206-213 (Player.py:57-68, :33-39, :78-89)
  if constexpr (!FAST) {
    const double speed = clamp_action((double)act.x), psp = (double)c.pspeed;
    const double nxf = __builtin_rint((double)px - (tm.s * psp) * speed);
    const double nyf = __builtin_rint((double)py - (tm.c * psp) * speed);
    const bool ok = (nxf >= 0.0) & (nxf + (double)c.psize <= (double)c.W) & (nyf >= 0.0) &
                    (nyf + (double)c.psize <= (double)c.H);
    px = ok ? (int)(ok ? nxf : 0.0) : px;
    py = ok ? (int)(ok ? nyf : 0.0) : py;
  } else {  // round_safe: rint(p - d) == p - rintf(d); player_pos_valid's bounds, safe against wrap
    // (selects on the wave-uniform `exact`, no branch: the tick's chain stays one block)
    const int nx = px - (PRE ? q.imx : (int)rintf(mdx)), ny = py - (PRE ? q.imy : (int)rintf(mdy));
    bool ok;
    if constexpr (STEADY) ok = skrange::fits_board(nx, ny, c.W - c.psize, c.H - c.psize);
    else ok = (nx >= 0) & (nx <= c.W - c.psize) & (ny >= 0) & (ny <= c.H - c.psize);
    px = exact ? epx : (ok ? nx : px);
    py = exact ? epy : (ok ? ny : py);
  }
  rot = rn;
  qx = f ? px : qx;
  qy = f ? py : qy;
  qrot = f ? rot : qrot;
  qvalid = f ? 1 : qvalid;
  qcd = f ? c.cdmax : qcd;
  qage = f ? 0 : qage;
  // game_tick  SkillshotGame.py:115-122 (Projectile.py:38-53); live is the same in both lanes
  const int lv = live != 0;
  ticks += lv;
  {
    const double qsp = (double)c.qspeed;
    int nx, ny;
    if constexpr (FAST) {
      // the step of this tick: a fired projectile's from the angle addition,
      // else the carried one; either way the flight's from here on
      const int sdx = f ? (PRE ? q.iex : (int)rintf(ex)) : tc.dx, sdy = f ? (PRE ? q.iey : (int)rintf(ey)) : tc.dy;
      tc.dx = sdx;
      tc.dy = sdy;
      tc.qex = f ? unq : tc.qex;
      tc.kq = f ? rn : tc.kq;
      nx = exact ? enx : qx - sdx;
      ny = exact ? eny : qy - sdy;
    } else {
      const int nxF = qx - (int)rintf(ex), nyF = qy - (int)rintf(ey);
      const int nxE = (int)__builtin_rint((double)qx - tt.s * qsp), nyE = (int)__builtin_rint((double)qy - tt.c * qsp);
      nx = fast ? nxF : nxE;
      ny = fast ? nyF : nyE;
    }
    bool ok;
    if constexpr (STEADY) ok = skrange::fits_board(nx, ny, c.W - c.qsize, c.H - c.qsize);
    else ok = (nx + c.qsize <= c.W) & (nx >= 0) & (ny + c.qsize <= c.H) & (ny >= 0);
    const bool upd = lv && qvalid;
    qx = (upd && ok) ? nx : qx;
    qy = (upd && ok) ? ny : qy;
    qvalid = (upd && !ok) ? 0 : qvalid;
    qcd -= lv;
    qage += lv;
  }
  // SkillshotGame.check_collision (:58-94): player 1 tested first
  int opx = 0, opy = 0;  // the other player's position (the observation's; the collision's in the 88-B forms)
  if constexpr (!PACK) {
    opx = pair_swap(px);
    opy = pair_swap(py);
  }
  int oqx, oqy, oqv;
  if constexpr (STEADY) {
    // The steady tick stores its state here, ahead of the collision test, with
    // `live` and `winner` as loaded: on a tick without a hit (all but about
    // one wave-tick in forty) that is the tick's result, and the test, its
    // three exchanges and the selects run behind the stores, in the stretch
    // the wave rests anyway.  A game hit in this tick is `done`: the cold
    // block below stores its {pos, cah} word again (the restart all three
    // planes), from the same lane to the same address in program order.
    oqv = pair_swap(qvalid);
    const bool qch = __double_as_longlong(qrot) != __double_as_longlong(q_old);
    const unsigned hi = p ? pack_flags(oqv, qvalid, live, winner) : (unsigned)ticks;
    if (in) split_store_pack<POL>(a, rp, L, rot, qrot, qch, pack_pos(px, py, qx, qy), pack_cah(qcd, qage, hi));
    if constexpr (kSteadyPrio) __builtin_amdgcn_s_setprio(0);  // (raised behind the state wait: steady_tick)
    __builtin_amdgcn_sched_barrier(0);  // (the test stays behind the stores)
    oqx = pair_swap(qx);
    oqy = pair_swap(qy);
  } else {
    oqx = pair_swap(qx);
    oqy = pair_swap(qy);
    oqv = pair_swap(qvalid);
  }
  if constexpr (PACK) {
    // the packed forms: one test per lane, "my player is hit by the partner's
    // projectile", and the pair exchanges the bit (skrange::pair_hit); the
    // steady tick's test in its one-compare form (sk_range.hpp)
    bool mine;
    if constexpr (STEADY) mine = (int)(oqv != 0) & (int)skrange::box_hit(px, py, c.psize, oqx, oqy, c.qsize);
    else mine = hit_test_s(c, px, py, oqx, oqy, oqv);
    const bool theirs = pair_swap((int)mine) != 0;
    const skrange::PairHit h = skrange::pair_hit(lv != 0, p ? theirs : mine, p ? mine : theirs);
    winner = h.h1 ? 1 : (h.h2 ? 2 : winner);
    live = ((int)h.h1 | (int)h.h2) ? 0 : live;
  } else {
    const int p1x = p ? opx : px, p1y = p ? opy : py, q1x = p ? oqx : qx, q1y = p ? oqy : qy, q1v = p ? oqv : qvalid;
    const int p2x = p ? px : opx, p2y = p ? py : opy, q2x = p ? qx : oqx, q2y = p ? qy : oqy, q2v = p ? qvalid : oqv;
    const bool h1 = lv && hit_test_s(c, p1x, p1y, q2x, q2y, q2v);
    const bool h2 = lv && !h1 && hit_test_s(c, p2x, p2y, q1x, q1y, q1v);
    winner = h1 ? 1 : (h2 ? 2 : winner);
    live = (h1 || h2) ? 0 : live;
  }
  // every load of this tick consumed (see multi_tick); a steady tick is never
  // the launch's last, and the generic tick that is settles the slot
  if constexpr (!STEADY) ctr_settle(wc);
  bool to_pack = STEADY;  // (a steady tick's wave was admitted for the launch: no fit test)
  if constexpr (PACK && !STEADY) {
    const bool fit = !in || ((int)pack_fits_player(px, py, qx, qy, qcd, qage, qvalid) &
                               (int)pack_fits_game(ticks, live, winner));
    to_pack = !last && __ballot(!fit) == 0;  // wave-uniform
    // admission to the steady loop for the `left` ticks after this one
    // (skrange::admit_*): no lane's state can stop fitting before they end
    const bool adm = !in || ((int)skrange::admit_player(px, py, qx, qy, qcd, qage, qvalid) &
                               (int)skrange::admit_game(ticks, live, winner, left));
    *admit = to_pack && __ballot(!adm) == 0;
  }
  if constexpr (STEADY) {
    // (stored above, ahead of the collision test)
  } else if (PACK && to_pack) {  // the packed halves out before done / restart
    const bool qch = (!STEADY && !packed) || __double_as_longlong(qrot) != __double_as_longlong(q_old);
    const unsigned hi = p ? pack_flags(oqv, qvalid, live, winner) : (unsigned)ticks;
    if (in) split_store_pack<POL>(a, rp, L, rot, qrot, qch, pack_pos(px, py, qx, qy), pack_cah(qcd, qage, hi));
  } else {  // the state out before done / restart (multi_compute's early store, for its reason)
    const unsigned fl = (unsigned)(qvalid & 0xff) | ((unsigned)(oqv & 0xff) << 8) | ((unsigned)(live & 0xff) << 16) |
                        ((unsigned)(winner & 0xff) << 24);
    const bool qch = STEADY || (PACK && packed) || __double_as_longlong(qrot) != __double_as_longlong(q_old);
    if (in) split_store_state<POL>(a, r, L, px, py, rot, qx, qy, qrot, qch, qcd, qage, ticks, fl);
  }
  bool amb = false;
  double gq = 0.0;  // the fast projectile gradient (the ambiguous flag's interval check)
  const int aqx = qx, aqy = qy;  // the post-tick projectile, for the flag's redo
  const double aqrot = qrot;
  if constexpr (OBS) {
    if (in) {  // prepare_states / calculate_rewards_* (SkillshotLearner.py:512-603) of the post-tick state
      float o[12], pd;
      obs12_sc(c, px, py, rot, pr, qx, qy, qrot, tq_obs, qcd, qvalid, opx, opy, o, &pd, &amb, &gq);
      if (a.obs) store_obs(a.obs + so * 24 * a.n, a.n, p, L.i, o);
      if (a.reward) {
        float rw;
        if (a.reward_kind == SK_REWARD_SIMPLE) {  // a difference of distances: fp64 roots
          const double mine = dist_point_point(qx, qy, opx, opy);
          const double theirs = dist_point_point(oqx, oqy, px, py);
          rw = (float)(mine - theirs);
        } else {
          rw = (float)(-(double)pd / (double)c.W);
        }
        a.reward[so * 2 * a.n + (int64_t)p * a.n + L.i] = rw;
      }
    }
  }
  const bool d = in && ((!live) || (ticks >= a.tick_limit));  // SkillshotLearner.py:302
  if (in && p == 0) {
    if constexpr (STEADY) {
      __builtin_amdgcn_raw_buffer_store_b8((unsigned char)d, ss->rd, ss->vd, ss->dso, 0);
      __builtin_amdgcn_raw_buffer_store_b8((unsigned char)winner, ss->rw, ss->vd, ss->dso, 0);
    } else {
      if (a.done) a.done[so * a.out_stride + L.i] = (uint8_t)d;
      if (a.winner) a.winner[so * a.out_stride + L.i] = (uint8_t)winner;
    }
  }
  bool any_done = true, rs = false;
  if constexpr (STEADY) any_done = __ballot(d) != 0;  // wave-uniform: the counts stay exact
  if (any_done) {
    const bool dc = d && p == 0;
    L.n_done += dc;
    L.n_h1 += dc && winner == 1;
    L.n_h2 += dc && winner == 2;
    L.t_sum += dc ? (unsigned)ticks : 0u;
    rs = d && a.auto_reset;  // SkillshotGame.__init__ :10-25 for this lane's player
    if (rs) {
      if (a.random_positions) {
        const U4 u4 = draw4(a.seed, (uint64_t)(a.env_offset + L.i), step, 1u);
        px = u32_to_pos(p ? u4.z : u4.x, c.rlo, c.rhi);
        py = u32_to_pos(p ? u4.w : u4.y, c.rlo, c.rhi);
      } else {
        px = p ? c.f2x : c.f1x;
        py = p ? c.f2y : c.f1y;
      }
      rot = 0.0; qx = 0; qy = 0; qrot = 0.0; qcd = 0; qage = 0; qvalid = 0;
      ticks = 0; live = 1; winner = 0;
    }
    const int ov = pair_swap(qvalid);  // every lane active (top level, or under the wave-uniform ballot)
    if (PACK && to_pack) {
      const unsigned hi = p ? pack_flags(ov, qvalid, live, winner) : (unsigned)ticks;
      if (rs) split_store_pack<POL>(a, rp, L, rot, qrot, true, pack_pos(px, py, qx, qy), pack_cah(qcd, qage, hi));
      if constexpr (STEADY) {
        // a game hit in this tick that does not restart: its flags (player 2's
        // lane) went out above as loaded, the word again with the hit in it
        // (`ov` is its `oqv`: nothing of it was reset).  Done by the tick
        // limit alone, or dead before the tick: nothing to correct.
        if (d && !rs && lv && !live && p)
          split_store_pack_word<POL>(a, rp, L, pack_pos(px, py, qx, qy), pack_cah(qcd, qage, hi));
      }
    } else if (rs) {
      const unsigned fl = (unsigned)(qvalid & 0xff) | ((unsigned)(ov & 0xff) << 8) | ((unsigned)(live & 0xff) << 16) |
                          ((unsigned)(winner & 0xff) << 24);
      split_store_state<POL>(a, r, L, px, py, rot, qx, qy, qrot, true, qcd, qage, ticks, fl);
    }
  }
  if constexpr (PACK) packed = to_pack;
  if constexpr (OBS) {
    // the future-collision flag within its margin of an edge, settled after
    // this tick's state stores (k_step_split's tail rule): by the interval
    // check unless it depends on g's last bits (then the correctly rounded tan)
    if (amb && a.obs) {
      const int fi = future_flag_interval(c, aqx, aqy, opx, opy, gq);
      const float fv = fi >= 0 ? (float)fi : future_flag_cr(c, aqx, aqy, aqrot, opx, opy);
      a.obs[so * 24 * a.n + ((int64_t)p * a.n + L.i) * 12 + 11] = fv;
    }
    // the next tick's carried sincos, already evaluated: sincos(rn) for the
    // move (sincos(0) = (0, 1) after a restart), the projectile's after shoot
    tc.m = rs ? sktrig::SinCos{0.0, 1.0} : xn;
    tc.kr = rot;
    tc.tq = tq_obs;
    tc.kq = qrot;
    tc.have = true;
  } else if (STEADY || !last) {  // the tick's final rotation: the next tick's carried sincos
    tc.pr = rot;
    if constexpr (!FAST) tc.qs = same_bits(qrot, rot);
    tc.pend = true;
  }
}

// BLK 512 (the 65,536-game geometry): one workgroup of 8 waves per CU, so
// each SIMD hosts waves w and w + 4 of ONE workgroup (MI355X_MICROARCH.md
// "Two waves per SIMD"); `stagger` > 0 starts waves 4-7 stagger x 512
// cycles late, so the pair alternates a tick's memory round trip with the
// partner's arithmetic instead of both waiting at once.
// PACK: the packed resident form between the ticks (split_tick_carry): 3 x 8
// bytes per lane and tick each way in place of 6, so at two waves per SIMD
// the tick is no longer bound by the fabric's bandwidth.  A compile-time
// form: the 88-B instantiations carry no branch for it.
// FAST: the step-only tick on fp32 trig with the exact fallback
// (split_tick_carry), also a compile-time form.
template <int POL, int BLK, bool OBS = false, int PF = 0, bool PACK = false, bool FAST = false>
__global__ void __launch_bounds__(BLK + (PF > 0 ? 64 : 0)) k_step_split_multi(MultiArgs a, Cfg c, int stagger) {
  if constexpr (PF > 0) {  // the action-slab prefetch wave (k_step_multi)
    __shared__ int4 pf_scratch[64];
    if (threadIdx.x >= BLK) {
      prefetch_wave<BLK / 2, PF>(a, pf_scratch);
      return;
    }
  }
  SplitLane L;
  const int64_t gt = (int64_t)blockIdx.x * BLK + threadIdx.x;
  L.i = gt >> 1;
  L.p = (int)(gt & 1);
  L.in = L.i < a.n;
  L.ic = L.in ? L.i : 0;
  L.hc = 2 * L.ic + L.p;
  L.h = 2 * L.i + L.p;
  L.n_done = L.n_h1 = L.n_h2 = L.t_sum = 0;
  if (stagger > 0 && (threadIdx.x >> 6) >= (BLK >> 7))
    for (int k = 0; k < stagger; ++k) __builtin_amdgcn_s_sleep(8);
  WaveCtr wc = ctr_load<BLK>(a.ctr);
  const uint64_t step0 = step_read(a.step);
  step_advance(a.step, step0, (uint64_t)a.n_ticks);
  const __amdgpu_buffer_rsrc_t r = raw_rsrc(a.base), rp = PACK ? raw_rsrc(a.pack) : r;
  bool packed = false;  // every launch starts from (and ends in) the exchange format
  bool admitted = false;  // PACK: the wave stays in the packed form for the rest of the launch (skrange::admit_*)
  int64_t slab = a.slab0, so = a.out0;
  // the slab one tick ahead in the register pair this tick does not read,
  // two ticks per iteration (k_step_multi's action pipeline)
  const int64_t aoff = (int64_t)L.p * a.n + L.ic;
  float2 pa0 = load_action(a.actions + slab * 2 * a.n + aoff), pa1;
  int64_t pslab = slab + 1 == a.ring ? 0 : slab + 1;
  typename SplitCarrySel<FAST>::type tc;
  tc.have = tc.pend = false;
  int t = 0;
  auto one_tick = [&](const float2& cur, float2& nxt) {
    SplitRaw w;
    if constexpr (PF > 0) __builtin_amdgcn_s_barrier();  // the prefetch wave (full contract at 512 lanes)
    if (PACK && packed) split_load_pack<POL>(a, rp, L, w);
    else split_load_raw<POL>(a, r, L, w);
    const int64_t ls = t + 1 < a.n_ticks ? pslab : slab;  // unconditional (see k_step_multi)
    nxt = load_action(a.actions + ls * 2 * a.n + aoff);
    __builtin_amdgcn_sched_barrier(0);
    // the last tick's rotation, while this tick's loads fly: hidden at one
    // wave per SIMD, paid in issue slots with co-resident waves (FAST: 32
    // VALU, 9 of them fp64, against 89 and 50)
    if (tc.pend) split_carry_advance(tc);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (PACK)
      split_tick_carry<POL, OBS, PACK, FAST>(a, c, r, L, wc, so, step0 + (uint64_t)t, w, cur, tc, t + 1 == a.n_ticks,
                                             rp, packed, nullptr, nullptr, a.n_ticks - 1 - t, &admitted);
    else
      split_tick_carry<POL, OBS, PACK, FAST>(a, c, r, L, wc, so, step0 + (uint64_t)t, w, cur, tc, t + 1 == a.n_ticks,
                                             rp, packed);
    slab = slab + 1 == a.ring ? 0 : slab + 1;
    pslab = pslab + 1 == a.ring ? 0 : pslab + 1;
    so = so + 1 == a.out_slabs ? 0 : so + 1;
  };
  if constexpr (PACK) {
    // The launch peeled: tick 0 (exchange format in) and the last tick
    // (exchange format out) run the generic tick above; between them, while
    // for a wave admitted for the rest of the launch, the steady loop: packed
    // in and out, not the last tick, the carry pending (split_tick_carry's
    // STEADY form), the ring and the output rows at 32-bit byte offsets
    // (a.steady32: the host checked that they fit) with one scalar add and
    // compare each per tick.  Admission (skrange::admit_*, balloted in the
    // generic tick on its post-tick state): no state of the wave can stop
    // fitting the packed form in the ticks that remain, so the loop is a
    // plain tick count with no fit test and no way out.  A wave that is not
    // admitted runs the generic tick, which still packs per tick while the
    // state fits, and asks again after every even tick.
    SplitSteady S;
    const uint32_t slab_b = (uint32_t)a.n * 16u, ring_b = (uint32_t)a.ring * slab_b;
    const uint32_t out_b = (uint32_t)a.out_slabs * (uint32_t)a.out_stride;
    S.ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<float2*>(a.actions), (short)0, (int)ring_b, 0x00020000);
    // (readfirstlane: the record counts in SGPRs, or the stores get a waterfall loop)
    S.rd = __builtin_amdgcn_make_buffer_rsrc(a.done, (short)0, __builtin_amdgcn_readfirstlane(a.done ? -1 : 0),
                                             0x00020000);
    S.rw = __builtin_amdgcn_make_buffer_rsrc(a.winner, (short)0, __builtin_amdgcn_readfirstlane(a.winner ? -1 : 0),
                                             0x00020000);
    S.va = (uint32_t)aoff * 8u;
    S.vd = (uint32_t)L.ic;
    S.aso = S.dso = 0;
    S.maybe = 0;
    const unsigned long long in_mask = __ballot(L.in);
    const bool full_wave = in_mask == ~0ull;  // wave-uniform
    auto steady_tick = [&](auto full, const float2& cur, float2& nxt) __attribute__((always_inline)) {
      SplitRaw w;
      split_load_pack<POL>(a, rp, L, w);
      const skb2i na = __builtin_amdgcn_raw_buffer_load_b64(S.ra, S.va, S.aso, 2);  // nontemporal, as load_action
      nxt = make_float2(__int_as_float(na.x), __int_as_float(na.y));
      __builtin_amdgcn_sched_barrier(0);
      split_carry_advance(tc);  // the last tick's rotation, while this tick's loads fly
      split_carry_pin(tc);
      // FAST: what the tick computes from the carry and the action alone,
      // also while the loads fly (about 55 VALU off the chain behind the
      // wait: 65,536 games 1.59-1.61 against 1.65-1.67 us per tick;
      // profiles/r12_bench_ab.jsonl).  The action came a tick ahead, so the
      // wait in front of it is for this wave's previous stores, which the
      // state loads' own wait implies anyway.
      SplitPre pre{};
      if constexpr (FAST) {
        pre = split_fast_pre(tc.m, tc.mok, cur, c);
        const unsigned long long unsafe = split_pre_pin(pre);
        S.maybe = split_pre_maybe(unsafe, tc.qex, decltype(full)::value ? ~0ull : in_mask);
      }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (kSteadyPrio) {
        // The chain from here to the last state store at issue priority 1
        // (split_tick_carry lowers it behind the stores).  The empty asm
        // takes the loaded state: the state wait stands in front of it, so
        // the wave does not wait at the raised priority.
        asm volatile("" : "+v"(w.rot.x), "+v"(w.rot.y), "+v"(w.qrot.x), "+v"(w.qrot.y), "+v"(w.pp.x), "+v"(w.pp.y));
        __builtin_amdgcn_s_setprio(1);
        __builtin_amdgcn_sched_barrier(0);
      }
      split_tick_carry<POL, false, true, FAST, true, decltype(full)::value>(a, c, r, L, wc, 0, step0 + (uint64_t)t, w,
                                                                            cur, tc, false, rp, packed, &S, &pre);
      // The wave rests kSteadyRest x 64 cycles between its stores and the
      // next tick's loads of the same lines.  With the loop's shorter tail
      // the reload followed the write-through stores within ~50 instructions
      // and waited far longer for them (1.89-1.90 us per tick against the
      // parent's 1.74-1.77: fewer slots, more wait); the generic tick's
      // done / store maze had kept the two apart.  A sleeping wave leaves
      // the issue port to its partner, which filler instructions would not
      // (0: 1.89, 3: 1.77, 4: 1.72, 5: 1.68, 6: 1.66-1.67, 7: 1.65-1.66,
      // 10: 1.71 us; profiles/r11_steady_rest_sweep.txt; with SplitPre under
      // the loads 0: 1.81, 3: 1.69, 4: 1.64, 5: 1.60, 6: 1.57, 7: 1.56-1.57,
      // 8: 1.57-1.58, 10: 1.58-1.59; profiles/r12_rest_sweep.jsonl; with the
      // collision test behind the stores and the chain at priority 1 the tail
      // rests for the wave: 2: 1.36, 3: 1.36-1.37, 4: 1.37-1.39, 5: 1.39,
      // 6: 1.40-1.41, 7: 1.39-1.40, 8: 1.43; profiles/r16_rest_sweep.jsonl).  The fp64-carry
      // form (the launches under kFastSplitMinTicks ticks) does not rest: its
      // 20-tick launch reads the parent's figure without, and 3.7 % more with
      // (profiles/r11_bench_ab_norest.jsonl, r11_bench_ab_rest_both.jsonl).
      if constexpr (FAST) __builtin_amdgcn_s_sleep(kSteadyRest);
      S.aso = S.aso + slab_b == ring_b ? 0u : S.aso + slab_b;
      S.dso = S.dso + (uint32_t)a.out_stride == out_b ? 0u : S.dso + (uint32_t)a.out_stride;
    };
    do {  // n_ticks >= 1 (host-checked); t is even here and this tick's actions are in pa0
      one_tick(pa0, pa1);
      if (++t >= a.n_ticks) break;
      if (a.steady32 && admitted && t + 2 < a.n_ticks) {
        const int t_in = t;
        const uint32_t slab_in = (uint32_t)slab, so_in = (uint32_t)so;
        S.aso = (uint32_t)pslab * slab_b;
        S.dso = so_in * (uint32_t)a.out_stride;
        // The loop's own action pair, cut from pa0 / pa1 by empty asms at its
        // entry and exit: sharing their registers left a copy of the pair on
        // the back edge, behind an s_waitcnt vmcnt(0), i.e. every second tick
        // waited for the wave's own state stores to be acknowledged.
        float2 sa0 = pa0, sa1 = pa1;
        asm volatile("" : "+v"(sa1.x), "+v"(sa1.y));
        auto steady_turns = [&](auto full) __attribute__((always_inline)) {
          do {  // two steady ticks per turn: neither is the launch's last; a plain tick count
            steady_tick(full, sa1, sa0);
            ++t;  // (the tick's RNG step counts from t)
            steady_tick(full, sa0, sa1);
            ++t;
          } while (t + 2 < a.n_ticks);
        };
        // A wave with all 64 lanes in range (every wave but at most the
        // launch's last) runs the loop's FULL form, without the lane mask
        // around the key check, the stores and the done rows;
        // the partial wave keeps the masked steady tick.
        if (full_wave) steady_turns(std::true_type{});
        else steady_turns(std::false_type{});
        pa0 = sa0;
        pa1 = sa1;
        asm volatile("" : "+v"(pa0.x), "+v"(pa0.y), "+v"(pa1.x), "+v"(pa1.y));
        // back to the generic tick's 64-bit ring positions (steady32: both fit 32 bits)
        const uint32_t dt = (uint32_t)(t - t_in);
        slab = (int64_t)((slab_in + dt) % (uint32_t)a.ring);
        pslab = slab + 1 == a.ring ? 0 : slab + 1;
        so = (int64_t)((so_in + dt) % (uint32_t)a.out_slabs);
      }
      one_tick(pa1, pa0);
    } while (++t < a.n_ticks);
  } else {
    do {  // n_ticks >= 1 (host-checked)
      one_tick(pa0, pa1);
      if (++t >= a.n_ticks) break;
      one_tick(pa1, pa0);
    } while (++t < a.n_ticks);
  }
  if (a.ctr) {
    const unsigned c4[4] = {L.n_done, L.n_h1, L.n_h2, L.t_sum};
    uint64_t v[4];
    wave_sum4_u32(c4, v);
    ctr_store<BLK>(a.ctr, wc, v[0], v[1], v[2], v[3]);
  }
}

template <typename... P, typename... A>
static hipError_t launch(void (*k)(P...), dim3 grid, dim3 block, hipStream_t s, A... args) {
  k<<<grid, block, 0, s>>>(args...);
  return hipGetLastError();
}

// k_step_split_multi<POL, BLK, OBS> with its action-slab prefetch wave pf
// ticks ahead (1, 2 or 4; 0 none; write-through port only)
// PACK (step-only, a.pack set): the packed resident form, no prefetch wave
// FAST (step-only): the fp32-trig tick
template <int POL, int BLK, bool OBS, bool PACK = false, bool FAST = false>
static hipError_t launch_split_multi(int pf, dim3 g, hipStream_t hs, const MultiArgs& a, const Cfg& c, int stagger) {
  if constexpr (PACK)
    return launch(k_step_split_multi<POL, BLK, false, 0, true, FAST>, g, dim3(BLK), hs, a, c, stagger);
  if constexpr (POL == 1) {
    if (pf == 1) return launch(k_step_split_multi<1, BLK, OBS, 1, false, FAST>, g, dim3(BLK + 64), hs, a, c, stagger);
    if (pf == 2) return launch(k_step_split_multi<1, BLK, OBS, 2, false, FAST>, g, dim3(BLK + 64), hs, a, c, stagger);
    if (pf > 2) return launch(k_step_split_multi<1, BLK, OBS, 4, false, FAST>, g, dim3(BLK + 64), hs, a, c, stagger);
  }
  return launch(k_step_split_multi<POL, BLK, OBS, 0, false, FAST>, g, dim3(BLK), hs, a, c, stagger);
}
// ... by workgroup width and state port
template <bool OBS, bool PACK, bool FAST>
static hipError_t launch_split_geom(bool wide, int pol, int pf, dim3 g512, dim3 g64, hipStream_t hs,
                                    const MultiArgs& a, const Cfg& c, int sg) {
  return wide ? (pol == 1 ? launch_split_multi<1, 512, OBS, PACK, FAST>(pf, g512, hs, a, c, sg)
                          : launch_split_multi<0, 512, OBS, PACK, FAST>(pf, g512, hs, a, c, sg))
              : (pol == 1 ? launch_split_multi<1, kStepBlock, OBS, PACK, FAST>(pf, g64, hs, a, c, sg)
                          : launch_split_multi<0, kStepBlock, OBS, PACK, FAST>(pf, g64, hs, a, c, sg));
}

// k_step_multi<POL, PACK, BLK> with its feed wave pf ticks ahead (1, 2 or 4;
// 0 none; only the write-through port's 88-B form on 64-lane workgroups has one)
template <int POL, bool PACK, int BLK>
static hipError_t launch_multi(int pf, hipStream_t hs, const MultiArgs& a, const Cfg& c, int early) {
  const dim3 g((unsigned)((a.n + BLK - 1) / BLK));
  if constexpr (POL == 1 && !PACK && BLK == kStepBlock) {
    if (pf == 1) return launch(k_step_multi<1, false, BLK, 1>, g, dim3(BLK + 64), hs, a, c, early);
    if (pf == 2) return launch(k_step_multi<1, false, BLK, 2>, g, dim3(BLK + 64), hs, a, c, early);
    if (pf > 2) return launch(k_step_multi<1, false, BLK, 4>, g, dim3(BLK + 64), hs, a, c, early);
  }
  return launch(k_step_multi<POL, PACK, BLK>, g, dim3(BLK), hs, a, c, early);
}

#endif  // SK_MULTI_HPP
