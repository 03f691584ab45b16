// sk_engine.hip — libskillshot: batched Skillshot env kernels for gfx950 and
// the C ABI declared in include/skillshot.h.
//
// Step kernels (the SoA planes of include/skillshot.h moved 16 bytes per game,
// or 8 per player, per load / store):
//   one tick per launch (sk_env_step; SK_STEP_VARIANT)
//     k_step              one lane per game, fp64 trig: do_actions x2 +
//                         game_tick + obs / reward + done / winner + masked
//                         auto-reset
//     k_step_split        two lanes per game, one per player (small batches)
//     k_step_fast         fp32 trig with an exact fp64 redo (large batches)
//   n ticks per launch (sk_env_step_multi, sk_env_step_multi_obs;
//   SK_MULTI_*): k_step_multi (one lane per game) and k_step_split_multi
//   (two), their state ports, packed resident form, split tick and launchers
//   live in sk_multi.hpp, which this file includes as part of its one
//   translation unit
//   k_rollout_random      n ticks of the random policy in one launch, state
//                         held in registers, in-kernel Philox actions
// Around them: k_gen_actions (random-policy actions into HBM), k_bot_act (a
// scripted actor's actions on the current state, sk_bot.hpp), k_reset /
// k_move_* / k_shoot / k_game_tick / k_observe / k_features (the reference's
// per-method API, batched), and the host side of the C ABI, which chooses
// among the kernels above.  For the multi-tick step that choice is a pure
// function in sk_multi_plan.hpp (plan_multi: geometry, workgroup, pack,
// prefetch, trig form); step_multi here validates, plans, gets the pack
// buffer, fills the arguments and hands the plan to launch_plan.
// Episode counters: wavefront ballots + popcount into one 128-B slot line per
// wave, read-modify-written without atomics (sk_step.hpp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "sk_device.hpp"
#include "sk_host.hpp"
#include "sk_multi_plan.hpp"
#include "sk_range.hpp"
#include "sk_stats.hpp"
#include "sk_step.hpp"


using namespace sk;

struct sk_env {
  int32_t n;
  int64_t env_offset;
  uint64_t seed;
  int32_t device;
  sk_config cfg;
  Cfg dcfg;
  View view;
  sk_state_view hview;
  bool owned;
  char* d_aux;               // [step slots: 256 B][counter slots]
  sk_counters* d_counters;   // counter_slots(n) slots: one per step-kernel wave
  // RNG step counter, device-resident so every call is hipGraph-capturable:
  // two slots ping-pong; a kernel reads slots[parity] and block 0 writes
  // slots[1-parity] = value + advance, then the host flips parity.
  uint64_t* d_step;
  int parity;
  // fused-step kernel: 0 = k_step (one lane per env, fp64 trig), 1 = k_step_split
  // (player per lane), 2 = k_step_fast (fp32 trig + exact fallback); -1 = auto
  // (SK_STEP_VARIANT overrides)
  int step_variant;
  skplan::MultiKnobs knobs;  // the SK_MULTI_* knobs (sk_multi_plan.hpp)
  char* d_pack;  // its scratch (48 B x n): make_env for the sizes that pack by default, else the first packed launch
  // device = -1: the CPU backend (sk_host.cpp) owns the games; every entry
  // point below forwards to it and takes host pointers
  skh::Host* host;
};

static thread_local std::string g_err;

static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                                 \
  do {                                                                                \
    hipError_t _e = (expr);                                                           \
    if (_e != hipSuccess)                                                             \
      return fail(SK_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e));       \
  } while (0)

static constexpr int kBlock = 256;
static constexpr int64_t kFastStepMinEnvs = 196608;
static constexpr int64_t kFastStepMaxEnvs = 786432;
// at or below this many games the step-only tick is latency-bound on a
// fraction of the SIMDs, and two lanes per game (k_step_split, half the
// dependent chain per lane) beat k_step: 8,192 games 3.25 vs 3.33 us, 16,384
// 3.58 vs 3.51 (profiles/r02_step_small_ab.jsonl) -- the per-GPU size of the
// metric's 65,536 games over 8 ranks
static constexpr int64_t kSplitStepMaxEnvs = 8192;
static constexpr int64_t kEarlyDrawMinEnvs = 32768;  // k_step: restart draw under the loads
// SK_CTR_STRIDE slots per wave of the widest step grid (k_step_split: two
// lanes per game), at least SK_COUNTER_SLOTS
static inline int64_t counter_slots(int64_t n) {
  // k_act_step32 counts one line per 16-game workgroup; the allocation keeps room for one per 8 games
  const int64_t w2 = (2 * n + 63) / 64, w8 = (n + 7) / 8, waves = w2 > w8 ? w2 : w8;
  return waves * SK_CTR_STRIDE > SK_COUNTER_SLOTS ? waves * SK_CTR_STRIDE : SK_COUNTER_SLOTS;
}
static inline size_t aux_bytes(int64_t n) { return 256 + (size_t)counter_slots(n) * sizeof(sk_counters); }

static inline unsigned grid_for(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }
static inline unsigned step_grid(int64_t n) { return (unsigned)((n + kStepBlock - 1) / kStepBlock); }

__device__ __forceinline__ float reward_of(const Cfg& c, const Env& e, int p, int kind, double path_dist) {
  if (kind == SK_REWARD_SIMPLE) {  // SkillshotLearner.py:600
    int o = 1 - p;
    double mine = dist_point_point(e.qx[p], e.qy[p], e.px[o], e.py[o]);
    double theirs = dist_point_point(e.qx[o], e.qy[o], e.px[p], e.py[p]);
    return (float)(mine - theirs);
  }
  return (float)(-path_dist / (double)c.W);  // SkillshotLearner.py:584
}

// ------------------------------------------------------------------ step trace
// Measurement build only (-DSK_TRACE_STEP; tools/trace_step.py): lane 0 of
// every k_step wave records s_memrealtime (100 MHz) at entry, once the loads
// have landed (a full s_waitcnt: perturbs the load/sincos overlap slightly),
// after the tick, and once its stores have completed, plus HW_ID / XCC_ID,
// into slot (step & 15) of sk_step_trace: [16][waves][8] u64.
#ifdef SK_TRACE_STEP
__device__ unsigned long long* sk_step_trace;
#define SK_TS(var) const unsigned long long var = __builtin_amdgcn_s_memrealtime()
#else
#define SK_TS(var)
#endif

// OBS: the launch writes obs / reward / obs_reset (instantiated apart so the
// step-only tick keeps no obs state live: holding the projectiles' sincos for
// the epilogue cost the headline tick 0.09 us, profiles/r02_step_obs_ab.jsonl)
template <bool OBS>
__global__ void __launch_bounds__(kStepBlock) k_step(StepArgs a, Cfg c) {
  int64_t i = (int64_t)blockIdx.x * kStepBlock + threadIdx.x;
  SK_TS(ts0);
  WaveCtr wc = ctr_load(a.ctr);
  const uint64_t step = step_read(a.step);
  step_advance(a.step, step, 1);
  bool in = i < a.n;
  bool d = false;
  Env e;
  double q_old0 = 0.0, q_old1 = 0.0;  // stored projectile rotations (store_env_q)
  sktrig::SinCos tq0 = {0.0, 1.0}, tq1 = {0.0, 1.0};  // the projectiles' sincos after shoot
  U4 ru = {0u, 0u, 0u, 0u};
#ifdef SK_TRACE_STEP
  unsigned long long ts1 = 0, ts2 = 0;
#endif
  if (in) {
    // state first, actions last (in issue order, so the waits for the state
    // do not wait for the actions): the players' sincos of the old rotations
    // then run while the actions arrive
    load_env(a.v, i, e);
    q_old0 = e.qrot[0];
    q_old1 = e.qrot[1];
    __builtin_amdgcn_sched_barrier(0);
    const float2 a0 = load_action(a.actions + i);
    const float2 a1 = load_action(a.actions + a.n + i);
    __builtin_amdgcn_sched_barrier(0);
    // the random restart's Philox draw (SkillshotGame.py:15 via :168) while
    // the state is in flight: the VALU is idle until it lands, whereas after
    // the tick the draw would sit on the finishing waves' tail (the empty asm
    // pins it here: it would otherwise be sunk into the restart branch).
    // Only for large grids: 4.30 -> 4.24 us at 65,536 games, but 3.28 ->
    // 3.34 us at 4,096, whose state lands before the draw is done
    // (profiles/r02_step_ablation.jsonl, run ed1)
    if (a.random_positions && a.n >= kEarlyDrawMinEnvs) {
      ru = draw4(a.seed, (uint64_t)(a.env_offset + i), step, 1u);
      asm volatile("" : "+v"(ru.x), "+v"(ru.y), "+v"(ru.z), "+v"(ru.w));
    }
    __builtin_amdgcn_sched_barrier(0);
#ifdef SK_TRACE_STEP
    __builtin_amdgcn_s_waitcnt(0);
    ts1 = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_sched_barrier(0);
#endif
    bool k0, k1;
    const sktrig::SinCos m0 = sktrig::sincos_bf(e.rot[0], &k0);
    const sktrig::SinCos m1 = sktrig::sincos_bf(e.rot[1], &k1);
    tick_env_m(c, e, m0, m1, k0 & k1, (double)a0.x, (double)a0.y, (double)a1.x, (double)a1.y, OBS ? &tq0 : nullptr,
               OBS ? &tq1 : nullptr);
#ifdef SK_TRACE_STEP
    __builtin_amdgcn_sched_barrier(0);
    ts2 = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_sched_barrier(0);
#endif
  }
  ctr_settle(wc);  // every load consumed, no state store issued yet
  float o0[12], o1[12];
  unsigned amb = 0;
  double g0 = 0.0, g1 = 0.0;  // the fast projectile gradients (fix_future_flags_g)
  if (in) {
    if (OBS && (a.obs || a.reward || a.obs_reset)) {
      float pd0, pd1;
      amb = obs_env_sc(c, e, tq0, tq1, o0, o1, &pd0, &pd1, &g0, &g1);
      if (a.obs) {
        store_obs(a.obs, a.n, 0, i, o0);
        store_obs(a.obs, a.n, 1, i, o1);
        if (amb) fix_future_flags_g(c, e, amb, g0, g1, a.obs, a.n, i);
      }
      if (a.reward) {
        a.reward[i] = reward_of(c, e, 0, a.reward_kind, (double)pd0);
        a.reward[a.n + i] = reward_of(c, e, 1, a.reward_kind, (double)pd1);
      }
    }
    d = (!e.live) || (e.ticks >= a.tick_limit);  // SkillshotLearner.py:302
    if (a.done) a.done[i] = (uint8_t)d;
    if (a.winner) a.winner[i] = (uint8_t)e.winner;
  }
  const int fin_winner = in ? e.winner : 0, fin_ticks = in ? e.ticks : 0;  // before the restart
  if (in && d && a.auto_reset) {
    if (a.random_positions) {
      if (a.n >= kEarlyDrawMinEnvs) reset_random_u(c, e, ru);
      else reset_random(c, e, a.seed, (uint64_t)(a.env_offset + i), step);
    }
    else reset_fixed(c, e);
  }
  if (OBS && in && a.obs_reset) {
    // a game that did not restart acts next on the obs just computed; a
    // restarted one on its fresh state's (rotations 0: sin 0, cos 1)
    if (d && a.auto_reset) {
      float pd0, pd1;
      amb = obs_env_sc(c, e, sktrig::SinCos{0.0, 1.0}, sktrig::SinCos{0.0, 1.0}, o0, o1, &pd0, &pd1);
    }
    store_obs(a.obs_reset, a.n, 0, i, o0);
    store_obs(a.obs_reset, a.n, 1, i, o1);
    if (amb) fix_future_flags_g(c, e, amb, g0, g1, a.obs_reset, a.n, i);  // (restarted: amb = 0)
  }
  if (in) store_env_q(a.v, i, e, q_old0, q_old1);
  if (a.ctr) wave_count(a.ctr, wc, d, fin_winner, fin_ticks);
  if (!in) return;
#ifdef SK_TRACE_STEP
  __builtin_amdgcn_s_waitcnt(0);
  const unsigned long long ts3 = __builtin_amdgcn_s_memrealtime();
  if ((threadIdx.x & 63) == 0 && sk_step_trace) {
    const unsigned waves = gridDim.x * (blockDim.x >> 6);
    const unsigned w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    unsigned long long* t = sk_step_trace + ((step & 15) * waves + w) * 8;
    t[0] = ts0; t[1] = ts1; t[2] = ts2; t[3] = ts3;
    t[4] = __builtin_amdgcn_s_getreg((31 << 11) | 4);   // HW_ID
    t[5] = __builtin_amdgcn_s_getreg((15 << 11) | 20);  // XCC_ID
  }
#endif
}

#ifdef SK_TRACE_STEP
extern "C" int skdiag_set_step_trace(void* buf) {
  return hipMemcpyToSymbol(HIP_SYMBOL(sk_step_trace), &buf, sizeof(buf)) == hipSuccess ? 0 : -1;
}
#endif

// Fused step, fp32-trig variant (SK_STEP_VARIANT=2; the default from 196,608
// games): the same tick through tick_env_fast (exact by construction: fp32
// deltas decide the rounding unless within their error bound of a tie, then
// the lane redoes the tick in fp64), with the loads issued by inline asm in
// arrival order (issue_step_loads).  ~35 % fewer VALU instructions; faster
// where several waves share a SIMD (8.9 vs 9.4 us per launch at 262,144
// games), slower than k_step at one wave per SIMD (65,536 games: 5.3 vs 4.7
// us), where the per-wave dependency chain, not issue, sets the time
// (profiles/r01g_step_variants.jsonl).
__global__ void __launch_bounds__(kStepBlock) k_step_fast(StepArgs a, Cfg c) {
  int64_t i = (int64_t)blockIdx.x * kStepBlock + threadIdx.x;
  bool in = i < a.n;
  // every load issued back to back before anything else touches memory,
  // then the tick works through the data in arrival order
  // (issue_step_loads: rotations -> players' sincos, projectile rotations ->
  // theirs, rest of the state -> decode, actions -> the tick)
  StepLoads L;
  if (in) issue_step_loads(a.v, a.actions, a.n, i, L);
  WaveCtr wc = ctr_load(a.ctr);
  bool d = false;
  Env e;
  if (in) {
    wait_rot(L);
    bool k0, k1, k2, k3;
    sktrig::SinCosF m0 = sktrig::sincos_fast(L.r.x, &k0);
    sktrig::SinCosF m1 = sktrig::sincos_fast(L.r.y, &k1);
    wait_qrot(L, m0, m1);
    sktrig::SinCosF tq0 = sktrig::sincos_fast(L.qr.x, &k2);
    sktrig::SinCosF tq1 = sktrig::sincos_fast(L.qr.y, &k3);
    wait_state(L, tq0, tq1);
    decode_env(step_loads_env(L), e);
    wait_actions(L);
    tick_env_fast(c, e, m0, m1, tq0, tq1, k0 & k1, k2, k3, L.a0.x, L.a0.y, L.a1.x, L.a1.y);
  }
  ctr_settle(wc);  // every load consumed, no state store issued yet
  if (in) {
    if (a.obs || a.reward) {
      float o0[12], o1[12];
      double pd0, pd1;
      const unsigned amb = obs_env(c, e, o0, o1, &pd0, &pd1);
      if (a.obs) {
        store_obs(a.obs, a.n, 0, i, o0);
        store_obs(a.obs, a.n, 1, i, o1);
        if (amb) fix_future_flags(c, e, amb, a.obs, a.n, i);
      }
      if (a.reward) {
        a.reward[i] = reward_of(c, e, 0, a.reward_kind, pd0);
        a.reward[a.n + i] = reward_of(c, e, 1, a.reward_kind, pd1);
      }
    }
    d = (!e.live) || (e.ticks >= a.tick_limit);  // SkillshotLearner.py:302
    if (a.done) a.done[i] = (uint8_t)d;
    if (a.winner) a.winner[i] = (uint8_t)e.winner;
  }
  if (!in) return;
  const int fin_winner = e.winner, fin_ticks = e.ticks;  // before the restart
  // the RNG step slot is read only by the waves that need it (all lanes
  // reading one line every launch made that line's L2 channel a hot spot)
  if (blockIdx.x == 0 && threadIdx.x == 0) step_advance(a.step, step_read(a.step), 1);
  if (d && a.auto_reset) {
    if (a.random_positions) reset_random(c, e, a.seed, (uint64_t)(a.env_offset + i), step_read(a.step));
    else reset_fixed(c, e);
  }
  if (a.obs_reset) {
    float o0[12], o1[12];
    double pd0, pd1;
    const unsigned amb = obs_env(c, e, o0, o1, &pd0, &pd1);
    store_obs(a.obs_reset, a.n, 0, i, o0);
    store_obs(a.obs_reset, a.n, 1, i, o1);
    if (amb) fix_future_flags(c, e, amb, a.obs_reset, a.n, i);
  }
  store_env_q(a.v, i, e, L.qr.x, L.qr.y);
  if (a.ctr) wave_count(a.ctr, wc, d, fin_winner, fin_ticks);  // after the stores (see wave_count)
}

// Player-split fused step: lanes (2i, 2i+1) own players 1 and 2 of env i.
// Each lane loads only its player's half of every plane (8-byte lanes, the
// pair covering the env's 16 bytes: still fully coalesced), runs that
// player's do_actions and projectile tick (a player's actions never read the
// other player), then the pair swaps positions/projectiles with one
// pair_swap (DPP) each for the collision test, which both lanes evaluate
// identically.  Twice the waves of k_step, half the dependent chain per lane.
__global__ void __launch_bounds__(kStepBlock) k_step_split(StepArgs a, Cfg c) {
  const int64_t gt = (int64_t)blockIdx.x * kStepBlock + threadIdx.x;
  sk_counters* slot = a.ctr ? ctr_slot(a.ctr) : nullptr;
  const StepLane L = split_load(a, gt, slot);
  // Loads are unconditional (split_load): issued rotation first, action
  // last, the player's sincos of its old rotation then runs while the rest
  // arrives
  __builtin_amdgcn_sched_barrier(0);
  const float2 act = load_action(a.actions + (int64_t)L.p * a.n + L.ic);
  __builtin_amdgcn_sched_barrier(0);
  split_finish(a, c, L, act, slot);
}

struct RolloutArgs {
  View v;
  int64_t n;
  int n_ticks;
  int tick_limit;
  uint64_t seed;
  int64_t env_offset;
  StepRef step;
  sk_counters* ctr;
};

__global__ void __launch_bounds__(kStepBlock) k_rollout_random(RolloutArgs a, Cfg c) {
  int64_t i = (int64_t)blockIdx.x * kStepBlock + threadIdx.x;
  bool in = i < a.n;
  const uint64_t step0 = step_read(a.step);
  step_advance(a.step, step0, (uint64_t)a.n_ticks);
  WaveCtr wc = ctr_load(a.ctr);
  Env e;
  if (in) load_env(a.v, i, e);
  uint64_t genv = (uint64_t)(a.env_offset + i);
  unsigned dones = 0, w1 = 0, w2 = 0;
  uint64_t tsum = 0;
  ctr_settle(wc);  // with the state loads, before any store
  if (in) {
    for (int t = 0; t < a.n_ticks; ++t) {
      uint64_t step = step0 + (uint64_t)t;
      U4 u = draw4(a.seed, genv, step, 0u);
      tick_env_fast(c, e, u32_to_action(u.x), u32_to_action(u.y), u32_to_action(u.z), u32_to_action(u.w));
      if ((!e.live) || (e.ticks >= a.tick_limit)) {
        dones += 1;
        w1 += (e.winner == 1);
        w2 += (e.winner == 2);
        tsum += (uint64_t)e.ticks;
        reset_random(c, e, a.seed, genv, step);
      }
    }
    store_env(a.v, i, e);
  }
  if (a.ctr) {
    uint64_t vals[4] = {dones, w1, w2, tsum};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      uint64_t x = vals[k];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
      vals[k] = x;
    }
    if (vals[0]) ctr_store(a.ctr, wc, vals[0], vals[1], vals[2], vals[3]);
  }
}

#include "sk_multi.hpp"  // the multi-tick step: k_step_multi, k_step_split_multi and their launchers

__global__ void __launch_bounds__(kBlock) k_gen_actions(float4* out, int64_t n, int n_ticks, uint64_t seed,
                                                        int64_t env_offset, StepRef sref) {
  const uint64_t step0 = step_read(sref);
  // out: [T][2][N] float2 viewed as pairs; each lane writes both players' float2
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  float2* o = reinterpret_cast<float2*>(out);
  for (int t = 0; t < n_ticks; ++t) {
    U4 u = draw4(seed, (uint64_t)(env_offset + i), step0 + (uint64_t)t, 0u);
    o[(int64_t)t * 2 * n + i] = make_float2(u32_to_action(u.x), u32_to_action(u.y));
    o[(int64_t)t * 2 * n + n + i] = make_float2(u32_to_action(u.z), u32_to_action(u.w));
  }
}

// sk_env_bot_act: both seats' scripted actions of one kind, lanes (2i, 2i + 1)
// of a wave owning players 1 and 2 of game i as in k_step_split (bot_lane
// reads the opponent through the pair exchange).  A lane past the end reads
// game 0 and stores nothing.
__global__ void __launch_bounds__(kStepBlock) k_bot_act(View v, int64_t n, int kind, float2* actions, Cfg c,
                                                        uint64_t seed, int64_t env_offset, StepRef sref) {
  const int64_t gt = (int64_t)blockIdx.x * kStepBlock + threadIdx.x, i = gt >> 1;
  const int p = (int)(gt & 1);
  const bool in = i < n;
  const int64_t hc = 2 * (in ? i : 0) + p;
  const int2 pp = reinterpret_cast<const int2*>(v.pos)[hc];
  const double rot = reinterpret_cast<const double*>(v.rot)[hc];
  const float2 a = bot_lane(kind, p, pp, rot, c, seed, (uint64_t)(env_offset + i), step_read(sref));
  if (in) actions[(int64_t)p * n + i] = a;
}

// sk_env_stats_tick: one tick of the match statistics (csrc/sk_stats.hpp) from
// the current state, k_bot_act's lanes (the partner's position and projectile
// through the pair exchange, which every lane joins).  stats int32
// [SK_N_STATS + 2][2][n]: a lane whose game's alive byte is set reads its ten
// words, updates them and stores them back; every other lane (one past the
// end among them, which reads game 0) stores nothing.
__global__ void __launch_bounds__(kStepBlock) k_stats_tick(View v, int64_t n, const uint8_t* __restrict__ alive,
                                                           int32_t* __restrict__ stats, Cfg c) {
  const int64_t gt = (int64_t)blockIdx.x * kStepBlock + threadIdx.x, i = gt >> 1;
  const int p = (int)(gt & 1);
  const bool in = i < n;
  const int64_t ic = in ? i : 0, hc = 2 * ic + p;
  const int2 pp = reinterpret_cast<const int2*>(v.pos)[hc];
  const int2 qq = reinterpret_cast<const int2*>(v.qpos)[hc];
  const int2 ca = reinterpret_cast<const int2*>(v.qcdage)[hc];
  const double rot = reinterpret_cast<const double*>(v.rot)[hc];
  const unsigned f = (unsigned)v.misc[ic].y;
  const int ox = pair_swap(pp.x), oy = pair_swap(pp.y), oqx = pair_swap(qq.x), oqy = pair_swap(qq.y);
  if (!in || !alive[ic]) return;
  int32_t* const w = stats + (int64_t)p * n + ic;  // word k of this (seat, game): w[2 n k]
  int32_t s[SK_N_STATS];
#pragma unroll
  for (int k = 0; k < SK_N_STATS; ++k) s[k] = w[2 * n * k];
  int32_t xp = w[2 * n * SK_N_STATS], yp = w[2 * n * (SK_N_STATS + 1)];
  const sktrig::SinCos m = skbot::sincos(rot, [](double x) { return sincos_lib(x); });
  skstat::tick(s, xp, yp, m, pp.x, pp.y, ox, oy, ca.x, ((f >> (8 * p)) & 0xff) != 0, ((f >> (8 * (1 - p))) & 0xff) != 0,
               oqx, oqy, c.psize, c.pspeed, c.W, c.H);
#pragma unroll
  for (int k = 0; k < SK_N_STATS; ++k) w[2 * n * k] = s[k];
  w[2 * n * SK_N_STATS] = xp;
  w[2 * n * (SK_N_STATS + 1)] = yp;
}

__global__ void __launch_bounds__(kBlock) k_reset(View v, int64_t n, const uint8_t* mask, int random,
                                                  uint64_t seed, int64_t env_offset, StepRef sref, Cfg c) {
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t step = step_read(sref);
  step_advance(sref, step, 1);
  if (i >= n || (mask && !mask[i])) return;
  Env e;
  if (random) reset_random(c, e, seed, (uint64_t)(env_offset + i), step);
  else reset_fixed(c, e);
  store_env(v, i, e);
}

__global__ void __launch_bounds__(kBlock) k_move_direction(View v, int64_t n, int p, const double* vals,
                                                           double scalar, Cfg c) {
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  Env e;
  load_env(v, i, e);
  double x = vals ? vals[i] : scalar;
  if (p == 0) move_direction(c, e, 0, x); else move_direction(c, e, 1, x);
  store_env(v, i, e);
}

__global__ void __launch_bounds__(kBlock) k_move_look(View v, int64_t n, int p, const double* vals,
                                                      double scalar, Cfg c) {
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  Env e;
  load_env(v, i, e);
  double x = vals ? vals[i] : scalar;
  if (p == 0) move_look(c, e, 0, x); else move_look(c, e, 1, x);
  store_env(v, i, e);
}

__global__ void __launch_bounds__(kBlock) k_move_discrete(View v, int64_t n, int p, int kind,
                                                          const uint8_t* mask, Cfg c) {
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n || (mask && !mask[i])) return;
  Env e;
  load_env(v, i, e);
  if (kind == 0) { if (p == 0) move_fwd_back(c, e, 0, false); else move_fwd_back(c, e, 1, false); }
  else if (kind == 1) { if (p == 0) move_fwd_back(c, e, 0, true); else move_fwd_back(c, e, 1, true); }
  else if (kind == 2) { if (p == 0) e.rot[0] += c.look; else e.rot[1] += c.look; }  // Player.py:27-28
  else { if (p == 0) e.rot[0] -= c.look; else e.rot[1] -= c.look; }                  // Player.py:30-31
  store_env(v, i, e);
}

__global__ void __launch_bounds__(kBlock) k_shoot(View v, int64_t n, int p, const uint8_t* mask, Cfg c) {
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n || (mask && !mask[i])) return;
  Env e;
  load_env(v, i, e);
  if (p == 0) shoot(c, e, 0); else shoot(c, e, 1);
  store_env(v, i, e);
}

__global__ void __launch_bounds__(kBlock) k_projectile_move(View v, int64_t n, int p, int tick,
                                                            const uint8_t* mask, Cfg c) {
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n || (mask && !mask[i])) return;
  Env e;
  load_env(v, i, e);
  if (p == 0) projectile_tick_s(c, e.qx[0], e.qy[0], e.qrot[0], e.qcd[0], e.qage[0], e.qvalid[0]);
  else projectile_tick_s(c, e.qx[1], e.qy[1], e.qrot[1], e.qcd[1], e.qage[1], e.qvalid[1]);
  if (!tick) {  // move_forwards alone: undo the tick's cooldown/age update
    if (p == 0) { e.qcd[0] += 1; e.qage[0] -= 1; } else { e.qcd[1] += 1; e.qage[1] -= 1; }
  }
  store_env(v, i, e);
}

__global__ void __launch_bounds__(kBlock) k_check_collision(View v, int64_t n, uint8_t* hit_out, Cfg c) {
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  Env e;
  load_env(v, i, e);
  int live = e.live, winner = e.winner;
  int hit_live = 1, hit = 0;
  collide_s(c, e.px[0], e.py[0], e.qx[0], e.qy[0], e.qvalid[0], e.px[1], e.py[1], e.qx[1], e.qy[1], e.qvalid[1],
            hit_live, hit);
  if (hit) { winner = hit; live = 0; }
  e.live = live;
  e.winner = winner;
  if (hit_out) hit_out[i] = (uint8_t)hit;
  store_env(v, i, e);
}

__global__ void __launch_bounds__(kBlock) k_game_tick(View v, int64_t n, Cfg c) {
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  Env e;
  load_env(v, i, e);
  game_tick(c, e);
  store_env(v, i, e);
}

__global__ void __launch_bounds__(kBlock) k_observe(View v, int64_t n, float* obs, float* reward, int kind,
                                                    Cfg c) {
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  Env e;
  load_env(v, i, e);
  float o0[12], o1[12];
  double pd0, pd1;
  const unsigned amb = obs_env(c, e, o0, o1, &pd0, &pd1);
  if (obs) {
    store_obs(obs, n, 0, i, o0);
    store_obs(obs, n, 1, i, o1);
    if (amb) fix_future_flags(c, e, amb, obs, n, i);
  }
  if (reward) {
    reward[i] = reward_of(c, e, 0, kind, pd0);
    reward[n + i] = reward_of(c, e, 1, kind, pd1);
  }
}

__global__ void __launch_bounds__(kBlock) k_features(View v, int64_t n, double* feat, Cfg c) {
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  Env e;
  load_env(v, i, e);
  for (int p = 0; p < 2; ++p) {
    double f[18];
    features18(c, e, p, f);
    double* d = feat + (i * 2 + p) * 18;
    for (int k = 0; k < 18; ++k) d[k] = f[k];
  }
}

// the board rasteriser's launch (sk_render.hip)
hipError_t sk_render_launch(const sk_config& cfg, const sk_state_view& view, const int64_t* ids, int64_t m,
                            uint8_t* out, hipStream_t stream);

// ------------------------------------------------------------------ host ABI
extern "C" {

const char* sk_last_error(void) { return g_err.c_str(); }

int sk_abi_version(void) { return SK_ABI_VERSION; }

void sk_config_default(sk_config* c) {
  if (!c) return;
  c->board_w = 250; c->board_h = 250;
  c->player_size = 5; c->projectile_size = 3;
  c->player_speed = 3; c->projectile_speed = 5;
  c->cooldown_max = 15; c->look_speed = 0.25;
  c->fixed_p1_x = 50; c->fixed_p1_y = 50;
  c->fixed_p2_x = 200; c->fixed_p2_y = 200;
  c->rand_lo = 25; c->rand_hi = 225;
}

static Cfg to_dcfg(const sk_config& s) {
  Cfg c;
  c.W = s.board_w; c.H = s.board_h; c.psize = s.player_size; c.qsize = s.projectile_size;
  c.pspeed = s.player_speed; c.qspeed = s.projectile_speed; c.cdmax = s.cooldown_max;
  c.look = s.look_speed;
  c.f1x = s.fixed_p1_x; c.f1y = s.fixed_p1_y; c.f2x = s.fixed_p2_x; c.f2y = s.fixed_p2_y;
  c.rlo = s.rand_lo; c.rhi = s.rand_hi;
  // (2 * (250 ** 2)) ** 0.5 : CPython float_pow -> libm pow(125000.0, 0.5)
  c.max_dist = std::pow(2.0 * (double)s.board_w * (double)s.board_w, 0.5);
  c.inv_max_dist = 1.0 / c.max_dist;
  c.inv_W = 1.0 / (double)s.board_w;
  c.inv_H = 1.0 / (double)s.board_h;
  c.inv_cdmax = 1.0 / (double)s.cooldown_max;
  c.fast_rot_max = look_fits_add(s.look_speed) ? kFastRotMax : -1.0;
  return c;
}

static int check_device(int32_t device) {
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count == 0) return fail(SK_ENODEV, "no HIP device available");
  if (device < 0 || device >= count) return fail(SK_EINVAL, "device index out of range");
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(SK_ENODEV, std::string("libskillshot is built for gfx950, device is ") + prop.gcnArchName);
  return SK_OK;
}

// The limits of sk_config (include/skillshot.h): what the
// kernels' int arithmetic holds without wrapping (skrange::kCfgMax = 2^20:
// sums of a few coordinates, sizes and steps stay far inside int; squared
// distances are taken in floating point), for both backends.
static int validate_cfg(const sk_config& c) {
  const int M = skrange::kCfgMax;
  const auto mag_ok = [](int v) { return v >= -M && v <= M; };
  if (c.board_w <= 0 || c.board_h <= 0 || c.player_size <= 0 || c.projectile_size <= 0 ||
      c.cooldown_max <= 0 || c.rand_hi <= c.rand_lo)
    return fail(SK_EINVAL, "invalid sk_config");
  if (c.board_w > M || c.board_h > M || c.cooldown_max > M || !mag_ok(c.player_speed) ||
      !mag_ok(c.projectile_speed) || !mag_ok(c.fixed_p1_x) || !mag_ok(c.fixed_p1_y) || !mag_ok(c.fixed_p2_x) ||
      !mag_ok(c.fixed_p2_y) || !mag_ok(c.rand_lo) || !mag_ok(c.rand_hi))
    return fail(SK_EINVAL, "sk_config: a board side, speed, cooldown or start position beyond 2^20");
  if (c.player_size > c.board_w || c.player_size > c.board_h || c.projectile_size > c.board_w ||
      c.projectile_size > c.board_h)
    return fail(SK_EINVAL, "sk_config: a box larger than the board");
  if (!(std::fabs(c.look_speed) <= 1048576.0))  // (also refuses NaN)
    return fail(SK_EINVAL, "sk_config: look_speed not finite or beyond 2^20");
  return SK_OK;
}

static int make_env(sk_env** out, const sk_state_view* view, int32_t n, int64_t env_offset, uint64_t seed,
                    int32_t device, const sk_config* cfg) {
  if (!out) return fail(SK_EINVAL, "out is NULL");
  *out = nullptr;
  if (n <= 0) return fail(SK_EINVAL, "n_envs must be > 0");
  if (device == -1) {  // CPU backend
    sk_env* e = new sk_env();
    e->n = n;
    e->env_offset = env_offset;
    e->seed = seed;
    e->device = -1;
    if (cfg) e->cfg = *cfg; else sk_config_default(&e->cfg);
    int rc0 = validate_cfg(e->cfg);
    if (rc0) { delete e; return rc0; }
    if (view && (view->n_envs != n || !view->pos || !view->rot || !view->qpos || !view->qrot || !view->qcdage ||
                 !view->misc)) {
      delete e;
      return fail(SK_EINVAL, "incomplete sk_state_view");
    }
    e->host = skh::create(n, env_offset, seed, e->cfg, view);
    if (!e->host) { delete e; return fail(SK_ENOMEM, "host state allocation"); }
    e->hview = skh::view_of(*e->host);
    e->owned = view == nullptr;
    *out = e;
    return SK_OK;
  }
  int rc = check_device(device);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(device));
  sk_env* e = new sk_env();
  e->n = n;
  e->env_offset = env_offset;
  e->seed = seed;
  e->device = device;
  if (cfg) e->cfg = *cfg; else sk_config_default(&e->cfg);
  if ((rc = validate_cfg(e->cfg))) { delete e; return rc; }
  e->dcfg = to_dcfg(e->cfg);
  e->parity = 0;
  e->step_variant = -1;
  if (const char* sv = std::getenv("SK_STEP_VARIANT")) e->step_variant = std::atoi(sv);
  e->knobs = skplan::multi_knobs_from_env();
  e->d_pack = nullptr;
  if (view) {
    if (view->n_envs != n || !view->pos || !view->rot || !view->qpos || !view->qrot || !view->qcdage ||
        !view->misc) {
      delete e;
      return fail(SK_EINVAL, "incomplete sk_state_view");
    }
    e->hview = *view;
    e->owned = false;
  } else {
    e->owned = true;
    e->hview.n_envs = n;
    void* p = nullptr;
    size_t bytes = (size_t)n * 88;
    if (hipMalloc(&p, bytes) != hipSuccess) { delete e; return fail(SK_ENOMEM, "hipMalloc state"); }
    char* b = (char*)p;  // 16-B planes first, int2 last: every plane stays 16-B aligned
    e->hview.pos = (int32_t*)b; b += (size_t)n * 16;
    e->hview.rot = (double*)b; b += (size_t)n * 16;
    e->hview.qpos = (int32_t*)b; b += (size_t)n * 16;
    e->hview.qrot = (double*)b; b += (size_t)n * 16;
    e->hview.qcdage = (int32_t*)b; b += (size_t)n * 16;
    e->hview.misc = (int32_t*)b;
  }
  e->view.pos = (int4*)e->hview.pos;
  e->view.rot = (double2*)e->hview.rot;
  e->view.qpos = (int4*)e->hview.qpos;
  e->view.qrot = (double2*)e->hview.qrot;
  e->view.qcdage = (int4*)e->hview.qcdage;
  e->view.misc = (int2*)e->hview.misc;
  for (void* p : {(void*)e->view.pos, (void*)e->view.rot, (void*)e->view.qpos, (void*)e->view.qrot,
                  (void*)e->view.qcdage}) {
    if (((uintptr_t)p) & 15) {
      if (e->owned) (void)hipFree(e->hview.pos);
      delete e;
      return fail(SK_EINVAL, "state planes must be 16-byte aligned");
    }
  }
  if (((uintptr_t)e->view.misc) & 7) {
    if (e->owned) (void)hipFree(e->hview.pos);
    delete e;
    return fail(SK_EINVAL, "misc plane must be 8-byte aligned");
  }
  if (hipMalloc(&e->d_aux, aux_bytes(n)) != hipSuccess) {
    if (e->owned) (void)hipFree(e->hview.pos);
    delete e;
    return fail(SK_ENOMEM, "hipMalloc counters");
  }
  HIP_TRY(hipMemset(e->d_aux, 0, aux_bytes(n)));
  e->d_step = reinterpret_cast<uint64_t*>(e->d_aux);
  e->d_counters = reinterpret_cast<sk_counters*>(e->d_aux + 256);
  // the packed form's scratch for the sizes that pack by default, so that no
  // multi-tick launch has to allocate (a capturing stream cannot); a failure
  // here leaves it to the first launch
  if (e->knobs.pack != 0 && (int64_t)n >= skplan::kSplitPackMinEnvs && (uint64_t)n * 48u <= 0xffffffffull) {
    if (hipMalloc(&e->d_pack, (size_t)n * 48) != hipSuccess) {
      e->d_pack = nullptr;
      (void)hipGetLastError();
    }
  }
  if (e->owned) {
    k_reset<<<grid_for(n), kBlock, 0, 0>>>(e->view, n, nullptr, 0, seed, env_offset, StepRef{e->d_step, 0},
                                           e->dcfg);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    // creation does not consume a step value
    HIP_TRY(hipMemset(e->d_step, 0, 2 * sizeof(uint64_t)));
    HIP_TRY(hipDeviceSynchronize());
  }
  *out = e;
  return SK_OK;
}

int sk_env_create(sk_env** out, int32_t n_envs, int64_t env_offset, uint64_t seed, int32_t device,
                  const sk_config* cfg) {
  return make_env(out, nullptr, n_envs, env_offset, seed, device, cfg);
}

int sk_env_attach(sk_env** out, const sk_state_view* view, int64_t env_offset, uint64_t seed, int32_t device,
                  const sk_config* cfg) {
  if (!view) return fail(SK_EINVAL, "view is NULL");
  return make_env(out, view, view->n_envs, env_offset, seed, device, cfg);
}

int sk_env_destroy(sk_env* e) {
  if (!e) return fail(SK_EINVAL, "NULL handle");
  if (e->host) {
    skh::destroy(e->host);
    delete e;
    return SK_OK;
  }
  (void)hipSetDevice(e->device);
  if (e->owned) (void)hipFree(e->hview.pos);
  (void)hipFree(e->d_aux);
  if (e->d_pack) (void)hipFree(e->d_pack);
  delete e;
  return SK_OK;
}

int sk_env_get_view(const sk_env* e, sk_state_view* out) {
  if (!e || !out) return fail(SK_EINVAL, "NULL argument");
  *out = e->hview;
  return SK_OK;
}

int sk_env_counters_ptr(const sk_env* e, sk_counters** out) {
  if (!e || !out) return fail(SK_EINVAL, "NULL argument");
  if (e->host) {  // one host slot
    *out = &e->host->ctr;
    return SK_OK;
  }
  *out = e->d_counters;
  return SK_OK;
}

int sk_env_counter_slots(const sk_env* e, int64_t* out) {
  if (!e || !out) return fail(SK_EINVAL, "NULL argument");
  *out = e->host ? 1 : counter_slots(e->n);
  return SK_OK;
}

// one workgroup sums every wave's slot line into a 32-byte result (ADVICE r02:
// read_counters copied the O(n) slot array to the host)
__global__ void __launch_bounds__(kBlock) k_sum_counters(const sk_counters* slots, int64_t ns, sk_counters* out) {
  __shared__ unsigned long long part[4][kBlock];
  unsigned long long s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  for (int64_t k = threadIdx.x; k < ns; k += kBlock) {
    const sk_counters v = slots[k];
    s0 += v.dones; s1 += v.hits_p1; s2 += v.hits_p2; s3 += v.ticks_sum;
  }
  part[0][threadIdx.x] = s0; part[1][threadIdx.x] = s1; part[2][threadIdx.x] = s2; part[3][threadIdx.x] = s3;
  __syncthreads();
  for (int w = kBlock / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      for (int j = 0; j < 4; ++j) part[j][threadIdx.x] += part[j][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = sk_counters{part[0][0], part[1][0], part[2][0], part[3][0]};
}

int sk_env_read_counters(sk_env* e, sk_counters* out, void* stream) {
  if (!e || !out) return fail(SK_EINVAL, "NULL argument");
  if (e->host) {
    *out = e->host->ctr;
    return SK_OK;
  }
  sk_counters* d_sum = reinterpret_cast<sk_counters*>(e->d_aux + 64);  // step slots use bytes 0-15
  k_sum_counters<<<1, kBlock, 0, (hipStream_t)stream>>>(e->d_counters, counter_slots(e->n), d_sum);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, d_sum, sizeof(sk_counters), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return SK_OK;
}

int sk_env_clear_counters(sk_env* e, void* stream) {
  if (!e) return fail(SK_EINVAL, "NULL handle");
  if (e->host) {
    e->host->ctr = sk_counters{0, 0, 0, 0};
    return SK_OK;
  }
  HIP_TRY(hipMemsetAsync(e->d_counters, 0, (size_t)counter_slots(e->n) * sizeof(sk_counters),
                         (hipStream_t)stream));
  return SK_OK;
}

// The step counter only grows (every launch stores value + advance >= value
// into the other slot), so the current value is the larger slot whatever
// parity the host believes in: a graph captured at one parity and replayed
// after an odd number of eager launches leaves the host parity stale, never
// the maximum.
int sk_env_get_step_counter(const sk_env* e, uint64_t* out) {
  if (!e || !out) return fail(SK_EINVAL, "NULL argument");
  if (e->host) {
    *out = e->host->step;
    return SK_OK;
  }
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  uint64_t s[2];
  HIP_TRY(hipMemcpy(s, e->d_step, sizeof(s), hipMemcpyDeviceToHost));
  *out = s[0] > s[1] ? s[0] : s[1];
  return SK_OK;
}

int sk_env_set_step_counter(sk_env* e, uint64_t v) {
  if (!e) return fail(SK_EINVAL, "NULL handle");
  if (e->host) {
    e->host->step = v;
    return SK_OK;
  }
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  const uint64_t s[2] = {v, v};
  HIP_TRY(hipMemcpy(e->d_step, s, sizeof(s), hipMemcpyHostToDevice));
  e->parity = 0;
  return SK_OK;
}

__global__ void k_sync_step_slots(uint64_t* slots) {
  if (threadIdx.x == 0) {
    const uint64_t a = slots[0], b = slots[1], m = a > b ? a : b;
    slots[0] = m;
    slots[1] = m;
  }
}

int sk_env_sync_step_counter(sk_env* e, void* stream) {
  if (!e) return fail(SK_EINVAL, "NULL handle");
  if (e->host) return SK_OK;  // one host counter: nothing to sync
  k_sync_step_slots<<<1, 64, 0, (hipStream_t)stream>>>(e->d_step);
  HIP_TRY(hipGetLastError());
  e->parity = 0;
  return SK_OK;
}

#define SK_CHECK_ENV(e) \
  if (!(e)) return fail(SK_EINVAL, "NULL handle")
#define SK_CHECK_PID(pid) \
  if ((pid) != 1 && (pid) != 2) return fail(SK_EINVAL, "player_id must be 1 or 2")
#define SK_LAUNCH_CHECK() HIP_TRY(hipGetLastError())

int sk_env_reset(sk_env* e, const uint8_t* mask, int32_t random_positions, void* stream) {
  SK_CHECK_ENV(e);
  if (e->host) return skh::reset(*e->host, mask, random_positions), SK_OK;
  k_reset<<<grid_for(e->n), kBlock, 0, (hipStream_t)stream>>>(e->view, e->n, mask, random_positions, e->seed,
                                                               e->env_offset, StepRef{e->d_step, e->parity}, e->dcfg);
  SK_LAUNCH_CHECK();
  e->parity ^= 1;
  return SK_OK;
}

int sk_player_move_direction(sk_env* e, int32_t pid, const double* speeds, double scalar, void* stream) {
  SK_CHECK_ENV(e);
  SK_CHECK_PID(pid);
  if (e->host) return skh::move_direction(*e->host, pid - 1, speeds, scalar), SK_OK;
  k_move_direction<<<grid_for(e->n), kBlock, 0, (hipStream_t)stream>>>(e->view, e->n, pid - 1, speeds, scalar,
                                                                        e->dcfg);
  SK_LAUNCH_CHECK();
  return SK_OK;
}

int sk_player_move_look(sk_env* e, int32_t pid, const double* angles, double scalar, void* stream) {
  SK_CHECK_ENV(e);
  SK_CHECK_PID(pid);
  if (e->host) return skh::move_look(*e->host, pid - 1, angles, scalar), SK_OK;
  k_move_look<<<grid_for(e->n), kBlock, 0, (hipStream_t)stream>>>(e->view, e->n, pid - 1, angles, scalar,
                                                                   e->dcfg);
  SK_LAUNCH_CHECK();
  return SK_OK;
}

int sk_player_move_discrete(sk_env* e, int32_t pid, int32_t kind, const uint8_t* mask, void* stream) {
  SK_CHECK_ENV(e);
  SK_CHECK_PID(pid);
  if (kind < 0 || kind > 3) return fail(SK_EINVAL, "kind must be 0..3");
  if (e->host) return skh::move_discrete(*e->host, pid - 1, kind, mask), SK_OK;
  k_move_discrete<<<grid_for(e->n), kBlock, 0, (hipStream_t)stream>>>(e->view, e->n, pid - 1, kind, mask,
                                                                       e->dcfg);
  SK_LAUNCH_CHECK();
  return SK_OK;
}

int sk_player_shoot(sk_env* e, int32_t pid, const uint8_t* mask, void* stream) {
  SK_CHECK_ENV(e);
  SK_CHECK_PID(pid);
  if (e->host) return skh::shoot(*e->host, pid - 1, mask), SK_OK;
  k_shoot<<<grid_for(e->n), kBlock, 0, (hipStream_t)stream>>>(e->view, e->n, pid - 1, mask, e->dcfg);
  SK_LAUNCH_CHECK();
  return SK_OK;
}

int sk_projectile_move(sk_env* e, int32_t pid, int32_t tick, const uint8_t* mask, void* stream) {
  SK_CHECK_ENV(e);
  SK_CHECK_PID(pid);
  if (e->host) return skh::projectile_move(*e->host, pid - 1, tick, mask), SK_OK;
  k_projectile_move<<<grid_for(e->n), kBlock, 0, (hipStream_t)stream>>>(e->view, e->n, pid - 1, tick, mask,
                                                                         e->dcfg);
  SK_LAUNCH_CHECK();
  return SK_OK;
}

int sk_game_check_collision(sk_env* e, uint8_t* hit_out, void* stream) {
  SK_CHECK_ENV(e);
  if (e->host) return skh::check_collision(*e->host, hit_out), SK_OK;
  k_check_collision<<<grid_for(e->n), kBlock, 0, (hipStream_t)stream>>>(e->view, e->n, hit_out, e->dcfg);
  SK_LAUNCH_CHECK();
  return SK_OK;
}

int sk_game_tick(sk_env* e, void* stream) {
  SK_CHECK_ENV(e);
  if (e->host) return skh::game_tick(*e->host), SK_OK;
  k_game_tick<<<grid_for(e->n), kBlock, 0, (hipStream_t)stream>>>(e->view, e->n, e->dcfg);
  SK_LAUNCH_CHECK();
  return SK_OK;
}

int sk_env_features(sk_env* e, double* feat, void* stream) {
  SK_CHECK_ENV(e);
  if (!feat) return fail(SK_EINVAL, "feat is NULL");
  if (e->host) return skh::features(*e->host, feat), SK_OK;
  k_features<<<grid_for(e->n), kBlock, 0, (hipStream_t)stream>>>(e->view, e->n, feat, e->dcfg);
  SK_LAUNCH_CHECK();
  return SK_OK;
}

int sk_env_observe(sk_env* e, float* obs, float* reward, int32_t kind, void* stream) {
  SK_CHECK_ENV(e);
  if (kind != SK_REWARD_LOOKING && kind != SK_REWARD_SIMPLE) return fail(SK_EINVAL, "bad reward_kind");
  if (((uintptr_t)obs) & 15) return fail(SK_EINVAL, "obs must be 16-byte aligned");
  if (!obs && !reward) return SK_OK;
  if (e->host) return skh::observe(*e->host, obs, reward, kind), SK_OK;
  k_observe<<<grid_for(e->n), kBlock, 0, (hipStream_t)stream>>>(e->view, e->n, obs, reward, kind, e->dcfg);
  SK_LAUNCH_CHECK();
  return SK_OK;
}

static int step_launch(sk_env* e, const float* actions, float* obs, float* reward, int32_t reward_kind,
                       uint8_t* done, uint8_t* winner, int32_t tick_limit, int32_t auto_reset,
                       int32_t random_positions, float* obs_reset, const float* acting_obs, float* ring,
                       int64_t capacity, int64_t* total, uint32_t* arrivals, int64_t* total_copy,
                       void* stream) {
  SK_CHECK_ENV(e);
  if (!actions) return fail(SK_EINVAL, "actions is NULL");
  if (((uintptr_t)actions) & 7) return fail(SK_EINVAL, "actions must be 8-byte aligned");
  if ((((uintptr_t)obs) & 15) || (((uintptr_t)obs_reset) & 15))
    return fail(SK_EINVAL, "obs buffers must be 16-byte aligned");
  if (reward_kind != SK_REWARD_LOOKING && reward_kind != SK_REWARD_SIMPLE)
    return fail(SK_EINVAL, "bad reward_kind");
  if (ring) {
    if (!obs || !reward || !acting_obs || !total || !arrivals)
      return fail(SK_EINVAL, "ring insert needs obs, reward, acting_obs, total and arrivals");
    if (capacity <= 0 || 2 * (int64_t)e->n > capacity) return fail(SK_EINVAL, "ring capacity below 2 N rows");
    if ((((uintptr_t)ring) & 15) || (((uintptr_t)acting_obs) & 15) || (((uintptr_t)total) & 7) ||
        (((uintptr_t)total_copy) & 7))
      return fail(SK_EINVAL, "ring / acting_obs must be 16-byte aligned, total / total_copy 8-byte");
  }
  if (e->host) {
    skh::step(*e->host, actions, obs, reward, reward_kind, done, winner, tick_limit, auto_reset, random_positions,
              obs_reset);
    if (ring) {  // sk_replay_insert's rows on the host ring (player-major [2N] order)
      const int64_t n = e->n, base = *total;
      for (int64_t r = 0; r < 2 * n; ++r) {
        float* dst = ring + ((base + r) % capacity) * 28;
        std::memcpy(dst, acting_obs + r * 12, 12 * sizeof(float));
        dst[12] = actions[2 * r];
        dst[13] = actions[2 * r + 1];
        dst[14] = reward[r];
        std::memcpy(dst + 15, obs + r * 12, 12 * sizeof(float));
        dst[27] = done ? (float)done[r % n] : 0.f;
      }
      *total = base + 2 * n;
      if (total_copy) *total_copy = base + 2 * n;
    }
    return SK_OK;
  }
  StepArgs a;
  a.v = e->view;
  a.n = e->n;
  a.actions = reinterpret_cast<const float2*>(actions);
  a.obs = obs;
  a.reward = reward;
  a.reward_kind = reward_kind;
  a.done = done;
  a.winner = winner;
  a.tick_limit = tick_limit;
  a.auto_reset = auto_reset;
  a.random_positions = random_positions;
  a.obs_reset = obs_reset;
  a.seed = e->seed;
  a.env_offset = e->env_offset;
  a.step = StepRef{e->d_step, e->parity};
  a.ctr = e->d_counters;
  a.acting_obs = acting_obs;
  a.ring = ring;
  a.ring_cap = capacity;
  a.ring_total = total;
  a.ring_arrivals = arrivals;
  a.ring_total_copy = ring ? total_copy : nullptr;
  a.grid_blocks = 0;
  // auto: k_step_fast once several waves share a SIMD (>= 2 per SIMD on 256
  // CUs) up to ~3 per SIMD (262,144 games: 8.3 vs 9.1 us); k_step from
  // 1 M games, where the step is HBM-bound (1 M: 30.1 vs 31.6 us, 4 M: 137
  // vs 151 us; profiles/r01x_sweep_qskip.jsonl); below 196,608 k_step, or
  // k_step_split when observations are written (65,536 games with obs: 9.8
  // vs 10.5 us; profiles/r01g_step_variants.jsonl, r01v_step_block_ab.jsonl).
  // The ring insert is k_step_split's.
  // A look step past sincos_add's range (look_fits_add): k_step_fast would
  // send every firing lane through its fp64 redo, so such a configuration
  // runs k_step where it would have run k_step_fast, forced or not.
  const int chosen = ring ? 1
                     : e->step_variant >= 0 ? e->step_variant
                     : (e->n >= kFastStepMinEnvs && e->n < kFastStepMaxEnvs) ? 2
                     : e->n >= kFastStepMaxEnvs ? 0
                     : (obs || reward || obs_reset || e->n <= kSplitStepMaxEnvs) ? 1 : 0;
  const int variant = chosen == 2 && !look_fits_add(e->cfg.look_speed) ? 0 : chosen;
  if (variant == 1)
    k_step_split<<<step_grid(2 * (int64_t)e->n), kStepBlock, 0, (hipStream_t)stream>>>(a, e->dcfg);
  else if (variant == 2)
    k_step_fast<<<step_grid(e->n), kStepBlock, 0, (hipStream_t)stream>>>(a, e->dcfg);
  else if (a.obs || a.reward || a.obs_reset)
    k_step<true><<<step_grid(e->n), kStepBlock, 0, (hipStream_t)stream>>>(a, e->dcfg);
  else
    k_step<false><<<step_grid(e->n), kStepBlock, 0, (hipStream_t)stream>>>(a, e->dcfg);
  SK_LAUNCH_CHECK();
  e->parity ^= 1;
  return SK_OK;
}

int sk_env_step(sk_env* e, const float* actions, float* obs, float* reward, int32_t reward_kind, uint8_t* done,
                uint8_t* winner, int32_t tick_limit, int32_t auto_reset, int32_t random_positions,
                float* obs_reset, void* stream) {
  return step_launch(e, actions, obs, reward, reward_kind, done, winner, tick_limit, auto_reset, random_positions,
                     obs_reset, nullptr, nullptr, 0, nullptr, nullptr, nullptr, stream);
}

int sk_env_step_insert(sk_env* e, const float* actions, float* obs, float* reward, int32_t reward_kind,
                       uint8_t* done, uint8_t* winner, int32_t tick_limit, int32_t auto_reset,
                       int32_t random_positions, float* obs_reset, const float* acting_obs, float* ring,
                       int64_t capacity, int64_t* total, uint32_t* arrivals, int64_t* total_copy,
                       void* stream) {
  if (!ring) return fail(SK_EINVAL, "ring is NULL");
  return step_launch(e, actions, obs, reward, reward_kind, done, winner, tick_limit, auto_reset, random_positions,
                     obs_reset, acting_obs, ring, capacity, total, arrivals, total_copy, stream);
}

// sk_env_act_step's checks and StepArgs (N % 4 == 0)
static int act_step_args(sk_env* e, const float* acting_obs, const float* actions, float* obs, float* reward,
                         int32_t reward_kind, uint8_t* done, uint8_t* winner, int32_t tick_limit, int32_t auto_reset,
                         int32_t random_positions, float* obs_reset, float* ring, int64_t capacity, int64_t* total,
                         uint32_t* arrivals, int64_t* total_copy, StepArgs& a) {
  if ((((uintptr_t)obs) & 15) || (((uintptr_t)obs_reset) & 15))
    return fail(SK_EINVAL, "obs buffers must be 16-byte aligned");
  if (reward_kind != SK_REWARD_LOOKING && reward_kind != SK_REWARD_SIMPLE) return fail(SK_EINVAL, "bad reward_kind");
  if (ring) {
    if (!obs || !reward || !total || !arrivals)
      return fail(SK_EINVAL, "ring insert needs obs, reward, total and arrivals");
    if (capacity <= 0 || 2 * (int64_t)e->n > capacity) return fail(SK_EINVAL, "ring capacity below 2 N rows");
    if ((((uintptr_t)ring) & 15) || (((uintptr_t)total) & 7) || (((uintptr_t)total_copy) & 7))
      return fail(SK_EINVAL, "ring must be 16-byte aligned, total / total_copy 8-byte");
  }
  a.v = e->view;
  a.n = e->n;
  a.actions = reinterpret_cast<const float2*>(actions);
  a.obs = obs;
  a.reward = reward;
  a.reward_kind = reward_kind;
  a.done = done;
  a.winner = winner;
  a.tick_limit = tick_limit;
  a.auto_reset = auto_reset;
  a.random_positions = random_positions;
  a.obs_reset = obs_reset;
  a.seed = e->seed;
  a.env_offset = e->env_offset;
  a.step = StepRef{e->d_step, e->parity};
  a.ctr = e->d_counters;
  a.acting_obs = acting_obs;
  a.ring = ring;
  a.ring_cap = capacity;
  a.ring_total = total;
  a.ring_arrivals = arrivals;
  a.ring_total_copy = ring ? total_copy : nullptr;
  a.grid_blocks = 0;
  return SK_OK;
}

static int act_step_common(sk_env* e, const float* actor_flat, const float* acting_obs, const float* actions) {
  SK_CHECK_ENV(e);
  if (e->host) return fail(SK_EINVAL, "sk_env_act_step runs on the GPU backend");
  if (!actor_flat || !acting_obs || !actions) return fail(SK_EINVAL, "actor_flat / acting_obs / actions is NULL");
  if ((((uintptr_t)actions) & 7) || (((uintptr_t)acting_obs) & 15))
    return fail(SK_EINVAL, "actions must be 8-byte aligned, acting_obs 16-byte");
  return SK_OK;
}

int sk_env_act_step(sk_env* e, const float* actor_flat, const void* actor_pack, const float* acting_obs,
                    float* actions, float noise_sd,
                    float action_sd, uint64_t noise_seed, uint64_t* call_counter, float* obs, float* reward,
                    int32_t reward_kind, uint8_t* done, uint8_t* winner, int32_t tick_limit, int32_t auto_reset,
                    int32_t random_positions, float* obs_reset, float* ring, int64_t capacity, int64_t* total,
                    uint32_t* arrivals, int64_t* total_copy, void* stream) {
  int rc = act_step_common(e, actor_flat, acting_obs, actions);
  if (rc != SK_OK) return rc;
  if (e->n % 4) {  // the fused tile keys its noise by aligned 4-row groups: two launches
    rc = sk_actor_forward_f32(actor_flat, actor_pack, acting_obs, actions, 2 * (int64_t)e->n, noise_sd, action_sd,
                              noise_seed, call_counter, stream);
    if (rc != SK_OK) return fail(rc, "sk_actor_forward_f32 failed");
    return step_launch(e, actions, obs, reward, reward_kind, done, winner, tick_limit, auto_reset,
                       random_positions, obs_reset, acting_obs, ring, capacity, total, arrivals, total_copy, stream);
  }
  StepArgs a;
  rc = act_step_args(e, acting_obs, actions, obs, reward, reward_kind, done, winner, tick_limit, auto_reset,
                     random_positions, obs_reset, ring, capacity, total, arrivals, total_copy, a);
  if (rc != SK_OK) return rc;
  rc = sk_launch_act_step32(actor_flat, actor_pack, actions, noise_sd, action_sd, noise_seed, call_counter, a,
                            e->dcfg, (hipStream_t)stream);
  if (rc != SK_OK) return fail(rc, "k_act_step32 launch failed");
  e->parity ^= 1;
  return SK_OK;
}

int sk_env_act_episode(sk_env* e, const float* actor_flat, const void* actor_pack, float* states, float* actions,
                       float* rewards, int32_t* lengths, int32_t n_ticks, float noise_sd, float action_sd,
                       uint64_t noise_seed, uint64_t* call_counter, int32_t reward_kind, int32_t tick_limit,
                       void* stream) {
  int rc = act_step_common(e, actor_flat, states, actions);
  if (rc != SK_OK) return rc;
  if (!rewards || !lengths || n_ticks <= 0) return fail(SK_EINVAL, "rewards / lengths NULL or n_ticks <= 0");
  if (e->n % 4) return fail(SK_EINVAL, "sk_env_act_episode needs N % 4 == 0");
  if (((uintptr_t)lengths) & 3) return fail(SK_EINVAL, "lengths must be 4-byte aligned");
  if (!actor_pack || (((uintptr_t)actor_pack) & 15)) return fail(SK_EINVAL, "actor_pack is NULL or misaligned");
  StepArgs a;
  rc = act_step_args(e, states, actions, states + (size_t)24 * e->n, rewards, reward_kind, nullptr, nullptr,
                     tick_limit, 0, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, a);
  if (rc != SK_OK) return rc;
  rc = sk_launch_act_episode32(actor_flat, actor_pack, noise_sd, action_sd, noise_seed, call_counter, a, e->dcfg,
                               states, actions, rewards, lengths, n_ticks, (hipStream_t)stream);
  if (rc != SK_OK) return fail(rc, "k_act_episode32 launch failed");
  e->parity ^= 1;
  return SK_OK;
}

// ---- sk_env_act_match / _league, their _rec twins and sk_env_act_step_pool refuse in one order (skillshot.h):
// the handle, every argument, the record and last, with all of those in order, a CPU-backend handle.
// the outputs of a match-shaped launch
static int match_out_check(const float* obs2, const float* returns, const int32_t* lengths, const int32_t* last_half,
                           int32_t n_ticks) {
  if (!obs2 || !lengths || n_ticks <= 0) return fail(SK_EINVAL, "obs2 or lengths is NULL, or n_ticks <= 0");
  if ((((uintptr_t)lengths) | ((uintptr_t)returns) | ((uintptr_t)last_half)) & 3)
    return fail(SK_EINVAL, "lengths / returns / last_half must be 4-byte aligned");
  if (((uintptr_t)obs2) & 15) return fail(SK_EINVAL, "obs2 must be 16-byte aligned");
  return SK_OK;
}

// a seating: n_pairs blocks of `block` games, each acting from its pair of the n_actors rows of nets
static int seating_check(const sk_env* e, const uint64_t* nets, int32_t n_actors, const int32_t* pairs,
                         int32_t n_pairs, int32_t block) {
  if (!nets || !pairs) return fail(SK_EINVAL, "the nets or the pairs table is NULL");
  if (n_actors < 1 || n_pairs < 1) return fail(SK_EINVAL, "n_actors and n_pairs must be at least 1");
  if (block <= 0 || block % 32) return fail(SK_EINVAL, "block must be a positive multiple of 32");
  if ((int64_t)e->n != (int64_t)n_pairs * block) return fail(SK_EINVAL, "the env must hold n_pairs * block games");
  if ((((uintptr_t)nets) & 7) || (((uintptr_t)pairs) & 3))
    return fail(SK_EINVAL, "nets must be 8-byte aligned, pairs 4-byte");
  return SK_OK;
}

// a match's StepArgs (checks reward_kind): each tick acts on one half of obs2 and writes the other, the two
// 96 N bytes apart; rewards into returns; no done / winner, no reset, no ring
static int match_step_args(sk_env* e, float* obs2, float* returns, int32_t reward_kind, int32_t tick_limit,
                           StepArgs& a) {
  return act_step_args(e, obs2, nullptr, obs2, returns, reward_kind, nullptr, nullptr, tick_limit, 0, 0, nullptr,
                       nullptr, 0, nullptr, nullptr, nullptr, a);
}

// a match record against its launch of `blocks` blocks of `block` games (include/skillshot.h)
static int rec_check(const sk_match_record* rec, int64_t blocks, int64_t block, int32_t n_ticks,
                     const float* returns) {
  if (!rec) return fail(SK_EINVAL, "rec is NULL");
  const sk_state_view& v = rec->states;
  if (!v.pos || !v.rot || !v.qpos || !v.qrot || !v.qcdage || !v.misc || !rec->actions)
    return fail(SK_EINVAL, "a plane of rec->states or rec->actions is NULL");
  if (rec->per_block < 1 || rec->per_block > block)
    return fail(SK_EINVAL, "rec->per_block must lie in [1, the block's games]");
  if ((int64_t)rec->rows != blocks * rec->per_block) return fail(SK_EINVAL, "rec->rows must be blocks * per_block");
  if (rec->slabs < 1 || (int64_t)v.n_envs != (int64_t)rec->slabs * rec->rows)
    return fail(SK_EINVAL, "rec->states.n_envs must be slabs * rows");
  if (rec->slab0 < 0) return fail(SK_EINVAL, "rec->slab0 must not be negative");
  if ((int64_t)rec->slab0 + n_ticks + 1 > rec->slabs)
    return fail(SK_EINVAL, "rec->slab0 + n_ticks + 1 slabs do not fit rec->slabs");
  if (rec->rewards && !returns) return fail(SK_EINVAL, "rec->rewards needs returns (no reward is computed without it)");
  if ((((uintptr_t)v.pos) | ((uintptr_t)v.rot) | ((uintptr_t)v.qpos) | ((uintptr_t)v.qrot) | ((uintptr_t)v.qcdage) |
       ((uintptr_t)v.misc)) & 7)
    return fail(SK_EINVAL, "the planes of rec->states must be 8-byte aligned");
  if ((((uintptr_t)rec->actions) | ((uintptr_t)rec->rewards)) & 3)
    return fail(SK_EINVAL, "rec->actions / rec->rewards must be 4-byte aligned");
  return SK_OK;
}

// sk_env_act_match (recording false: rec unused) and sk_env_act_match_rec
static int act_match(sk_env* e, const float* actor1_flat, const void* actor1_pack, const float* actor2_flat,
                     const void* actor2_pack, float* obs2, float* returns, int32_t* lengths, int32_t* last_half,
                     int32_t n_ticks, int32_t reward_kind, int32_t tick_limit, bool recording,
                     const sk_match_record* rec, void* stream) {
  SK_CHECK_ENV(e);
  if (!actor1_flat || !actor2_flat || !actor1_pack || !actor2_pack)
    return fail(SK_EINVAL, "an actor's flat or pack is NULL");
  if ((((uintptr_t)actor1_pack) | ((uintptr_t)actor2_pack)) & 15)
    return fail(SK_EINVAL, "actor1_pack / actor2_pack must be 16-byte aligned");
  StepArgs a;  // (the checks in the family's order)
  int rc = match_out_check(obs2, returns, lengths, last_half, n_ticks);
  if (rc == SK_OK) rc = match_step_args(e, obs2, returns, reward_kind, tick_limit, a);
  if (rc == SK_OK && recording) rc = rec_check(rec, 1, e->n, n_ticks, returns);
  if (rc != SK_OK) return rc;
  if (e->host) return fail(SK_EINVAL, "sk_env_act_match(_rec) runs on the GPU backend");
  rc = sk_launch_act_match32(actor1_flat, actor1_pack, actor2_flat, actor2_pack, a, e->dcfg, obs2, returns, lengths,
                             last_half, n_ticks, rec, (hipStream_t)stream);
  if (rc != SK_OK) return fail(rc, "k_act_match32(_rec) launch failed");
  e->parity ^= 1;
  return SK_OK;
}

int sk_env_act_match(sk_env* e, const float* actor1_flat, const void* actor1_pack, const float* actor2_flat,
                     const void* actor2_pack, float* obs2, float* returns, int32_t* lengths, int32_t* last_half,
                     int32_t n_ticks, int32_t reward_kind, int32_t tick_limit, void* stream) {
  return act_match(e, actor1_flat, actor1_pack, actor2_flat, actor2_pack, obs2, returns, lengths, last_half, n_ticks,
                   reward_kind, tick_limit, false, nullptr, stream);
}

int sk_env_act_match_rec(sk_env* e, const float* actor1_flat, const void* actor1_pack, const float* actor2_flat,
                         const void* actor2_pack, float* obs2, float* returns, int32_t* lengths, int32_t* last_half,
                         int32_t n_ticks, int32_t reward_kind, int32_t tick_limit, const sk_match_record* rec,
                         void* stream) {
  return act_match(e, actor1_flat, actor1_pack, actor2_flat, actor2_pack, obs2, returns, lengths, last_half, n_ticks,
                   reward_kind, tick_limit, true, rec, stream);
}

// sk_env_act_league and sk_env_act_league_rec, as act_match
static int act_league(sk_env* e, const uint64_t* nets, int32_t n_actors, const int32_t* pairs, int32_t n_pairs,
                      int32_t block, float* obs2, float* returns, int32_t* lengths, int32_t* last_half,
                      int32_t n_ticks, int32_t reward_kind, int32_t tick_limit, bool recording,
                      const sk_match_record* rec, void* stream, bool bots = false) {
  SK_CHECK_ENV(e);
  StepArgs a;
  int rc = seating_check(e, nets, n_actors, pairs, n_pairs, block);
  if (rc == SK_OK) rc = match_out_check(obs2, returns, lengths, last_half, n_ticks);
  if (rc == SK_OK) rc = match_step_args(e, obs2, returns, reward_kind, tick_limit, a);
  if (rc == SK_OK && recording) rc = rec_check(rec, n_pairs, block, n_ticks, returns);
  if (rc != SK_OK) return rc;
  if (e->host) return fail(SK_EINVAL, "sk_env_act_league(_rec) runs on the GPU backend");
  rc = (bots ? sk_launch_act_league32_bots : sk_launch_act_league32)(nets, n_actors, pairs, block, a, e->dcfg, obs2,
                                                                     returns, lengths, last_half, n_ticks, rec,
                                                                     (hipStream_t)stream);
  if (rc != SK_OK) return fail(rc, "k_act_league32(_rec) launch failed");
  e->parity ^= 1;
  return SK_OK;
}

int sk_env_act_league(sk_env* e, const uint64_t* nets, int32_t n_actors, const int32_t* pairs, int32_t n_pairs,
                      int32_t block, float* obs2, float* returns, int32_t* lengths, int32_t* last_half,
                      int32_t n_ticks, int32_t reward_kind, int32_t tick_limit, void* stream) {
  return act_league(e, nets, n_actors, pairs, n_pairs, block, obs2, returns, lengths, last_half, n_ticks, reward_kind,
                    tick_limit, false, nullptr, stream);
}

int sk_env_act_league_rec(sk_env* e, const uint64_t* nets, int32_t n_actors, const int32_t* pairs, int32_t n_pairs,
                          int32_t block, float* obs2, float* returns, int32_t* lengths, int32_t* last_half,
                          int32_t n_ticks, int32_t reward_kind, int32_t tick_limit, const sk_match_record* rec,
                          void* stream) {
  return act_league(e, nets, n_actors, pairs, n_pairs, block, obs2, returns, lengths, last_half, n_ticks, reward_kind,
                    tick_limit, true, rec, stream);
}

// sk_env_act_league_bots / _bots_rec: the same checks, the _bots kernels
int sk_env_act_league_bots(sk_env* e, const uint64_t* nets, int32_t n_actors, const int32_t* pairs, int32_t n_pairs,
                           int32_t block, float* obs2, float* returns, int32_t* lengths, int32_t* last_half,
                           int32_t n_ticks, int32_t reward_kind, int32_t tick_limit, void* stream) {
  return act_league(e, nets, n_actors, pairs, n_pairs, block, obs2, returns, lengths, last_half, n_ticks, reward_kind,
                    tick_limit, false, nullptr, stream, true);
}

int sk_env_act_league_bots_rec(sk_env* e, const uint64_t* nets, int32_t n_actors, const int32_t* pairs,
                               int32_t n_pairs, int32_t block, float* obs2, float* returns, int32_t* lengths,
                               int32_t* last_half, int32_t n_ticks, int32_t reward_kind, int32_t tick_limit,
                               const sk_match_record* rec, void* stream) {
  return act_league(e, nets, n_actors, pairs, n_pairs, block, obs2, returns, lengths, last_half, n_ticks, reward_kind,
                    tick_limit, true, rec, stream, true);
}

// sk_env_act_league_stats: act_league's checks (a record when one is given), then the stats buffer and the
// tallies' range, the _stats kernels
int sk_env_act_league_stats(sk_env* e, const uint64_t* nets, int32_t n_actors, const int32_t* pairs, int32_t n_pairs,
                            int32_t block, float* obs2, float* returns, int32_t* lengths, int32_t* last_half,
                            int32_t n_ticks, int32_t reward_kind, int32_t tick_limit, int32_t* stats,
                            const sk_match_record* rec, void* stream) {
  SK_CHECK_ENV(e);
  StepArgs a;
  int rc = seating_check(e, nets, n_actors, pairs, n_pairs, block);
  if (rc == SK_OK) rc = match_out_check(obs2, returns, lengths, last_half, n_ticks);
  if (rc == SK_OK) rc = match_step_args(e, obs2, returns, reward_kind, tick_limit, a);
  if (rc == SK_OK && rec) rc = rec_check(rec, n_pairs, block, n_ticks, returns);
  if (rc != SK_OK) return rc;
  if (!stats || (((uintptr_t)stats) & 3)) return fail(SK_EINVAL, "stats is NULL or not 4-byte aligned");
  if (!skstat::fits(tick_limit, e->cfg.board_w, e->cfg.board_h))
    return fail(SK_EINVAL, "tick_limit * max(board_w, board_h) must fit in int32 for the statistics");
  if (e->host) return fail(SK_EINVAL, "sk_env_act_league_stats runs on the GPU backend");
  rc = sk_launch_act_league32_stats(nets, n_actors, pairs, block, a, e->dcfg, obs2, returns, lengths, last_half,
                                    n_ticks, stats, rec, (hipStream_t)stream);
  if (rc != SK_OK) return fail(rc, "k_act_league32_stats launch failed");
  e->parity ^= 1;
  return SK_OK;
}

// sk_env_act_step_pool and sk_env_act_step_pool_bots
static int act_step_pool(sk_env* e, const uint64_t* nets, int32_t n_actors, const int32_t* pairs, int32_t n_pairs,
                         int32_t block, int32_t noisy_actor, const float* acting_obs, float* actions, float noise_sd,
                         float action_sd, uint64_t noise_seed, uint64_t* call_counter, float* obs, float* reward,
                         int32_t reward_kind, uint8_t* done, uint8_t* winner, int32_t tick_limit, int32_t auto_reset,
                         int32_t random_positions, float* obs_reset, float* ring, int64_t capacity, int64_t* total,
                         uint32_t* arrivals, int64_t* total_copy, void* stream, bool bots) {
  SK_CHECK_ENV(e);
  int rc = seating_check(e, nets, n_actors, pairs, n_pairs, block);
  if (rc != SK_OK) return rc;
  if (!acting_obs || !actions) return fail(SK_EINVAL, "acting_obs / actions is NULL");
  if (noisy_actor < -1 || noisy_actor >= n_actors) return fail(SK_EINVAL, "noisy_actor must lie in [-1, n_actors)");
  if ((((uintptr_t)actions) & 7) || (((uintptr_t)acting_obs) & 15))
    return fail(SK_EINVAL, "actions must be 8-byte aligned, acting_obs 16-byte");
  if (((uintptr_t)call_counter) & 7) return fail(SK_EINVAL, "call_counter must be 8-byte aligned");
  StepArgs a;
  rc = act_step_args(e, acting_obs, actions, obs, reward, reward_kind, done, winner, tick_limit, auto_reset,
                     random_positions, obs_reset, ring, capacity, total, arrivals, total_copy, a);
  if (rc != SK_OK) return rc;
  if (e->host) return fail(SK_EINVAL, "sk_env_act_step_pool runs on the GPU backend");
  rc = (bots ? sk_launch_act_step_pool32_bots : sk_launch_act_step_pool32)(
      nets, n_actors, pairs, block, noisy_actor, actions, noise_sd, action_sd, noise_seed, call_counter, a, e->dcfg,
      (hipStream_t)stream);
  if (rc != SK_OK) return fail(rc, "k_act_step_pool32 launch failed");
  e->parity ^= 1;
  return SK_OK;
}

int sk_env_act_step_pool(sk_env* e, const uint64_t* nets, int32_t n_actors, const int32_t* pairs, int32_t n_pairs,
                         int32_t block, int32_t noisy_actor, const float* acting_obs, float* actions, float noise_sd,
                         float action_sd, uint64_t noise_seed, uint64_t* call_counter, float* obs, float* reward,
                         int32_t reward_kind, uint8_t* done, uint8_t* winner, int32_t tick_limit, int32_t auto_reset,
                         int32_t random_positions, float* obs_reset, float* ring, int64_t capacity, int64_t* total,
                         uint32_t* arrivals, int64_t* total_copy, void* stream) {
  return act_step_pool(e, nets, n_actors, pairs, n_pairs, block, noisy_actor, acting_obs, actions, noise_sd, action_sd,
                       noise_seed, call_counter, obs, reward, reward_kind, done, winner, tick_limit, auto_reset,
                       random_positions, obs_reset, ring, capacity, total, arrivals, total_copy, stream, false);
}

int sk_env_act_step_pool_bots(sk_env* e, const uint64_t* nets, int32_t n_actors, const int32_t* pairs,
                              int32_t n_pairs, int32_t block, int32_t noisy_actor, const float* acting_obs,
                              float* actions, float noise_sd, float action_sd, uint64_t noise_seed,
                              uint64_t* call_counter, float* obs, float* reward, int32_t reward_kind, uint8_t* done,
                              uint8_t* winner, int32_t tick_limit, int32_t auto_reset, int32_t random_positions,
                              float* obs_reset, float* ring, int64_t capacity, int64_t* total, uint32_t* arrivals,
                              int64_t* total_copy, void* stream) {
  return act_step_pool(e, nets, n_actors, pairs, n_pairs, block, noisy_actor, acting_obs, actions, noise_sd, action_sd,
                       noise_seed, call_counter, obs, reward, reward_kind, done, winner, tick_limit, auto_reset,
                       random_positions, obs_reset, ring, capacity, total, arrivals, total_copy, stream, true);
}

static_assert(sizeof(ActStepJob) <= sizeof(sk_step_job), "sk_step_job too small for ActStepJob");

int sk_env_act_step_job(sk_env* e, const float* actor_flat, const void* actor_pack, const float* acting_obs,
                        float* actions, float noise_sd,
                        float action_sd, uint64_t noise_seed, uint64_t* call_counter, float* obs, float* reward,
                        int32_t reward_kind, uint8_t* done, uint8_t* winner, int32_t tick_limit, int32_t auto_reset,
                        int32_t random_positions, float* obs_reset, float* ring, int64_t capacity, int64_t* total,
                        uint32_t* arrivals, int64_t* total_copy, sk_step_job* job) {
  int rc = act_step_common(e, actor_flat, acting_obs, actions);
  if (rc != SK_OK) return rc;
  if (!job) return fail(SK_EINVAL, "job is NULL");
  if (e->n % 4) return fail(SK_EINVAL, "a prepared act_step needs N % 4 == 0 (use sk_env_act_step)");
  if (!actor_pack || (((uintptr_t)actor_pack) & 15)) return fail(SK_EINVAL, "actor_pack is NULL or misaligned");
  ActStepJob j;
  std::memset(&j, 0, sizeof(j));
  rc = act_step_args(e, acting_obs, actions, obs, reward, reward_kind, done, winner, tick_limit, auto_reset,
                     random_positions, obs_reset, ring, capacity, total, arrivals, total_copy, j.a);
  if (rc != SK_OK) return rc;
  j.magic = kActStepJobMagic;
  j.c = e->dcfg;
  j.aflat = actor_flat;
  j.apack = (const char*)actor_pack;
  j.act_out = actions;
  j.sd = noise_sd;
  j.action_sd = action_sd;
  j.seed = noise_seed;
  j.call_ctr = call_counter;
  std::memset(job, 0, sizeof(*job));
  std::memcpy(job, &j, sizeof(j));
  e->parity ^= 1;
  return SK_OK;
}

// the size arithmetic alone, for the tests (no device needed)
extern "C" int skdiag_split_steady_fits32(int64_t n, int64_t ring_slabs, int64_t out_slabs, int64_t out_stride) {
  return skplan::split_steady_fits32(n, ring_slabs, out_slabs, out_stride) ? 1 : 0;
}
// plan_multi alone, for the tests (no device needed).
// in[15]:  n, n_ticks, full, restart_fits, pack_allowed, planes_fit32, steady_ok, then the knobs policy, split,
//          early, block, stagger, prefetch, pack, fast
// out[12]: split, pol, blk, obs, pf, pack, fast, stagger, early, steady32, grid, block_threads
extern "C" int skdiag_multi_plan(const int64_t* in, int32_t* out) {
  if (!in || !out || in[0] <= 0 || in[1] <= 0) return SK_EINVAL;
  skplan::MultiPlanIn pi;
  pi.n = in[0];
  pi.n_ticks = (int)in[1];
  pi.full = in[2] != 0;
  pi.restart_fits = in[3] != 0;
  pi.pack_allowed = in[4] != 0;
  pi.planes_fit32 = in[5] != 0;
  pi.steady_ok = in[6] != 0;
  pi.knobs = {(int)in[7], (int)in[8], (int)in[9], (int)in[10], (int)in[11], (int)in[12], (int)in[13], (int)in[14]};
  const skplan::MultiPlan p = skplan::plan_multi(pi);
  const int32_t o[12] = {p.split, p.pol, p.blk, p.obs, p.pf, p.pack, p.fast, p.stagger, p.early, p.steady32,
                         (int32_t)p.grid, p.block_threads};
  std::memcpy(out, o, sizeof(o));
  return SK_OK;
}

// a MultiPlan's instantiation: the launchers of sk_multi.hpp by (OBS, PACK,
// FAST) or (BLK, PACK, POL); they pick the workgroup width, the port and the
// prefetch distance off the plan's effective values
static hipError_t launch_plan(const skplan::MultiPlan& p, hipStream_t hs, const MultiArgs& a, const Cfg& c) {
  if (p.split) {
    const dim3 g(p.grid);
    const bool wide = p.blk == 512;
    switch (p.obs << 2 | p.pack << 1 | (int)p.fast) {
      case 4: return launch_split_geom<true, false, false>(wide, p.pol, p.pf, g, g, hs, a, c, p.stagger);
      case 3: return launch_split_geom<false, true, true>(wide, p.pol, 0, g, g, hs, a, c, p.stagger);
      case 2: return launch_split_geom<false, true, false>(wide, p.pol, 0, g, g, hs, a, c, p.stagger);
      case 1: return launch_split_geom<false, false, true>(wide, p.pol, p.pf, g, g, hs, a, c, p.stagger);
      case 0: return launch_split_geom<false, false, false>(wide, p.pol, p.pf, g, g, hs, a, c, p.stagger);
    }
    return hipErrorInvalidValue;  // the full contract neither packs nor runs the fp32-trig tick
  }
  switch ((int)(p.blk == 256) << 2 | p.pack << 1 | p.pol) {
    case 7: return launch_multi<1, true, 256>(p.pf, hs, a, c, p.early);
    case 6: return launch_multi<0, true, 256>(p.pf, hs, a, c, p.early);
    case 5: return launch_multi<1, false, 256>(p.pf, hs, a, c, p.early);
    case 4: return launch_multi<0, false, 256>(p.pf, hs, a, c, p.early);
    case 3: return launch_multi<1, true, kStepBlock>(p.pf, hs, a, c, p.early);
    case 2: return launch_multi<0, true, kStepBlock>(p.pf, hs, a, c, p.early);
    case 1: return launch_multi<1, false, kStepBlock>(p.pf, hs, a, c, p.early);
    default: return launch_multi<0, false, kStepBlock>(p.pf, hs, a, c, p.early);
  }
}

// the write-through port reads the six planes through one buffer resource
// based at the lowest: they must lie within 4 GiB of it.  off[k] = plane k -
// lowest (pos, rot, qpos, qrot, qcdage, misc); *base = the lowest if they do
static bool planes_within_4gib(const sk_state_view& v, int64_t n, const char** base, uint32_t off[6]) {
  const char* p[6] = {(const char*)v.pos,  (const char*)v.rot,    (const char*)v.qpos,
                      (const char*)v.qrot, (const char*)v.qcdage, (const char*)v.misc};
  const char* lo = p[0];
  for (int k = 1; k < 6; ++k) lo = p[k] < lo ? p[k] : lo;
  bool ok = true;
  for (int k = 0; k < 6; ++k) {
    const uint64_t end = (uint64_t)(p[k] - lo) + (uint64_t)n * (k == 5 ? 8u : 16u);
    ok &= end <= 0xffffffffull;
    off[k] = (uint32_t)(p[k] - lo);
  }
  if (ok) *base = lo;
  return ok;
}

// sk_env_step_multi (obs == reward == NULL, full == false) and
// sk_env_step_multi_obs (full == true: the split geometry with the obs /
// reward epilogue, k_step_split_multi<POL, BLK, true>)
static int step_multi(sk_env* e, const float* actions, int64_t ring_slabs, int64_t slab0, int32_t n_ticks,
                      float* obs, float* reward, int32_t reward_kind, uint8_t* done, uint8_t* winner,
                      int64_t out_stride, int64_t out0, int64_t out_slabs, int32_t tick_limit, int32_t auto_reset,
                      int32_t random_positions, void* stream, bool full) {
  SK_CHECK_ENV(e);
  if (!actions) return fail(SK_EINVAL, "actions is NULL");
  if (((uintptr_t)actions) & 7) return fail(SK_EINVAL, "actions must be 8-byte aligned");
  if (n_ticks <= 0 || ring_slabs <= 0 || slab0 < 0 || slab0 >= ring_slabs || out_stride < 0)
    return fail(SK_EINVAL, "bad n_ticks / ring_slabs / slab0 / out_stride");
  if (out_slabs <= 0 || out0 < 0 || out0 >= out_slabs) return fail(SK_EINVAL, "bad out_slabs / out0");
  if (obs && (((uintptr_t)obs) & 15)) return fail(SK_EINVAL, "obs must be 16-byte aligned");
  if (full && reward_kind != SK_REWARD_LOOKING && reward_kind != SK_REWARD_SIMPLE)
    return fail(SK_EINVAL, "bad reward_kind");
  if (e->host) {
    const int64_t slab_floats = 4 * (int64_t)e->n, n = e->n;
    for (int32_t t = 0; t < n_ticks; ++t) {
      const int64_t s = (slab0 + t) % ring_slabs, so = (out0 + t) % out_slabs;
      skh::step(*e->host, actions + s * slab_floats, obs ? obs + so * 24 * n : nullptr,
                reward ? reward + so * 2 * n : nullptr, reward_kind, done ? done + so * out_stride : nullptr,
                winner ? winner + so * out_stride : nullptr, tick_limit, auto_reset, random_positions, nullptr);
    }
    return SK_OK;
  }
  if ((int64_t)e->n > (int64_t)0x7fffffff / 16) return fail(SK_EINVAL, "n_envs too large for k_step_multi");
  const hipStream_t hs = (hipStream_t)stream;
  const Cfg& dc = e->dcfg;
  MultiArgs a;
  a.base = nullptr;  // (the write-through port's resource: planes_within_4gib below)
  for (int k = 0; k < 6; ++k) a.off[k] = 0;

  // ---- what the plan reads
  skplan::MultiPlanIn pi;
  pi.n = e->n;
  pi.n_ticks = n_ticks;
  pi.full = full;
  pi.restart_fits =
      random_positions ? (dc.rlo >= 0 && dc.rhi <= 256)
                       : (((unsigned)dc.f1x | (unsigned)dc.f1y | (unsigned)dc.f2x | (unsigned)dc.f2y) < 256u);
  pi.pack_allowed = true;
  pi.planes_fit32 = true;
  if (e->knobs.policy == 1) pi.planes_fit32 = planes_within_4gib(e->hview, e->n, &a.base, a.off);
  // (and its integer range tests take their one-compare form: skrange::cfg_ok;
  // a wave stays in it for the rest of the launch: skrange::admit_cfg, with
  // the restart positions in a byte, which the packed kernel needs anyway:
  // restart_fits above)
  pi.steady_ok = skplan::split_steady_fits32(e->n, ring_slabs, out_slabs, out_stride) &&
                 skrange::cfg_ok(dc.W, dc.H, dc.psize, dc.qsize, dc.pspeed, dc.qspeed) &&
                 skrange::admit_cfg(dc.W, dc.H, dc.psize, dc.qsize, dc.cdmax);
  pi.knobs = e->knobs;
  // the fp32-trig instantiations take a fired projectile's step from
  // sincos_add: not for a look step past its range (look_fits_add), forced
  // (SK_MULTI_FAST=1) or not; the fp64-carry ones then evaluate it exactly
  // (Cfg::fast_rot_max)
  if (!look_fits_add(dc.look)) pi.knobs.fast = 0;

  // ---- the plan, and the pack buffer if it packs
  skplan::MultiPlan plan = skplan::plan_multi(pi);
  if (plan.pack && !e->d_pack) {
    // no allocation on a capturing stream: such a launch runs the 88-B form
    // (make_env allocates the buffer for the sizes that pack by default)
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(hs, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
      (void)hipGetLastError();
      pi.pack_allowed = false;
      plan = skplan::plan_multi(pi);
    } else if (hipMalloc(&e->d_pack, (size_t)e->n * 48) != hipSuccess) {
      return fail(SK_ENOMEM, "hipMalloc pack");
    }
  }

  // ---- the launch's arguments
  a.obs = full ? obs : nullptr;
  a.reward = full ? reward : nullptr;
  a.reward_kind = reward_kind;
  a.out0 = out0;
  a.out_slabs = out_slabs;
  a.v = e->view;
  a.n = e->n;
  a.actions = reinterpret_cast<const float2*>(actions);
  a.ring = ring_slabs;
  a.slab0 = slab0;
  a.n_ticks = n_ticks;
  a.steady32 = plan.steady32;
  a.done = done;
  a.winner = winner;
  a.out_stride = out_stride;
  a.tick_limit = tick_limit;
  a.auto_reset = auto_reset;
  a.random_positions = random_positions;
  a.seed = e->seed;
  a.env_offset = e->env_offset;
  a.step = StepRef{e->d_step, e->parity};
  a.ctr = e->d_counters;
  a.pack = plan.pack ? e->d_pack : nullptr;  // the packed resident form between the ticks
  const hipError_t err = launch_plan(plan, hs, a, dc);
  if (err != hipSuccess) return fail(SK_EHIP, std::string("k_step_multi launch: ") + hipGetErrorString(err));
  e->parity ^= 1;
  return SK_OK;
}

int sk_env_step_multi(sk_env* e, const float* actions, int64_t ring_slabs, int64_t slab0, int32_t n_ticks,
                      uint8_t* done, uint8_t* winner, int64_t out_stride, int32_t tick_limit, int32_t auto_reset,
                      int32_t random_positions, void* stream) {
  return step_multi(e, actions, ring_slabs, slab0, n_ticks, nullptr, nullptr, SK_REWARD_LOOKING, done, winner,
                    out_stride, 0, n_ticks > 0 ? n_ticks : 1, tick_limit, auto_reset, random_positions, stream, false);
}

int sk_env_step_multi_obs(sk_env* e, const float* actions, int64_t ring_slabs, int64_t slab0, int32_t n_ticks,
                          float* obs, float* reward, int32_t reward_kind, uint8_t* done, uint8_t* winner,
                          int64_t out_slabs, int64_t out0, int32_t tick_limit, int32_t auto_reset,
                          int32_t random_positions, void* stream) {
  SK_CHECK_ENV(e);
  return step_multi(e, actions, ring_slabs, slab0, n_ticks, obs, reward, reward_kind, done, winner, e->n, out0,
                    out_slabs, tick_limit, auto_reset, random_positions, stream, true);
}

int sk_gen_random_actions(sk_env* e, float* actions, int32_t n_ticks, void* stream) {
  SK_CHECK_ENV(e);
  if (!actions || n_ticks <= 0) return fail(SK_EINVAL, "bad actions / n_ticks");
  if (((uintptr_t)actions) & 7) return fail(SK_EINVAL, "actions must be 8-byte aligned");
  if (e->host) return skh::gen_random_actions(*e->host, actions, n_ticks), SK_OK;
  k_gen_actions<<<grid_for(e->n), kBlock, 0, (hipStream_t)stream>>>(
      reinterpret_cast<float4*>(actions), e->n, n_ticks, e->seed, e->env_offset, StepRef{e->d_step, e->parity});
  SK_LAUNCH_CHECK();
  return SK_OK;
}

// both seats' scripted actions of one kind (csrc/sk_bot.hpp) from the current state at the current step value:
// k_bot_act, two lanes per game like k_step_split; advances nothing
int sk_env_bot_act(sk_env* e, int32_t kind, float* actions, void* stream) {
  SK_CHECK_ENV(e);
  if (!actions) return fail(SK_EINVAL, "actions is NULL");
  if (!skbot::kind_ok(kind)) return fail(SK_EINVAL, "kind must be one of SK_BOT_STILL .. SK_BOT_CHASER");
  if (((uintptr_t)actions) & 7) return fail(SK_EINVAL, "actions must be 8-byte aligned");
  if (e->host) return skh::bot_act(*e->host, kind, actions), SK_OK;
  k_bot_act<<<step_grid(2 * (int64_t)e->n), kStepBlock, 0, (hipStream_t)stream>>>(
      e->view, e->n, kind, reinterpret_cast<float2*>(actions), e->dcfg, e->seed, e->env_offset,
      StepRef{e->d_step, e->parity});
  SK_LAUNCH_CHECK();
  return SK_OK;
}

// one tick of the match statistics (csrc/sk_stats.hpp) from the current state, for the games whose alive byte is set:
// k_stats_tick, two lanes per game like k_bot_act; advances nothing
int sk_env_stats_tick(sk_env* e, const uint8_t* alive, int32_t* stats, void* stream) {
  SK_CHECK_ENV(e);
  if (!alive || !stats) return fail(SK_EINVAL, "alive or stats is NULL");
  if (((uintptr_t)stats) & 3) return fail(SK_EINVAL, "stats must be 4-byte aligned");
  if (e->host) return skh::stats_tick(*e->host, alive, stats), SK_OK;
  k_stats_tick<<<step_grid(2 * (int64_t)e->n), kStepBlock, 0, (hipStream_t)stream>>>(e->view, e->n, alive, stats,
                                                                                     e->dcfg);
  SK_LAUNCH_CHECK();
  return SK_OK;
}

int sk_env_rollout_random(sk_env* e, int32_t n_ticks, int32_t tick_limit, void* stream) {
  SK_CHECK_ENV(e);
  if (n_ticks <= 0) return fail(SK_EINVAL, "n_ticks must be > 0");
  if (e->host) return skh::rollout_random(*e->host, n_ticks, tick_limit), SK_OK;
  RolloutArgs a;
  a.v = e->view;
  a.n = e->n;
  a.n_ticks = n_ticks;
  a.tick_limit = tick_limit;
  a.seed = e->seed;
  a.env_offset = e->env_offset;
  a.step = StepRef{e->d_step, e->parity};
  a.ctr = e->d_counters;
  k_rollout_random<<<step_grid(e->n), kStepBlock, 0, (hipStream_t)stream>>>(a, e->dcfg);
  SK_LAUNCH_CHECK();
  e->parity ^= 1;
  return SK_OK;
}

int sk_render_states(const sk_config* cfg, int32_t device, const sk_state_view* view, const int64_t* ids, int64_t m,
                     uint8_t* out, void* stream) {
  if (!view) return fail(SK_EINVAL, "view is NULL");
  if (!out) return fail(SK_EINVAL, "out is NULL");
  if (m < 0) return fail(SK_EINVAL, "m must be >= 0");
  if (((uintptr_t)out) & 15) return fail(SK_EINVAL, "out must be 16-byte aligned");
  sk_config c;
  if (cfg) c = *cfg; else sk_config_default(&c);
  if (c.board_w <= 0 || c.board_h <= 0 || (int64_t)c.board_w * c.board_h > 0x7fffffff)
    return fail(SK_EINVAL, "board_w x board_h must be in 1 .. 2^31 - 1 cells");
  if (c.player_size != 5 || c.projectile_size != 3)
    return fail(SK_EINVAL, "the board's sprites are the reference's: player_size 5, projectile_size 3");
  if (view->n_envs < 0 || !view->pos || !view->rot || !view->qpos || !view->qrot || !view->qcdage || !view->misc)
    return fail(SK_EINVAL, "incomplete sk_state_view");
  if (m == 0) return SK_OK;
  if (m > INT64_MAX / ((int64_t)c.board_w * c.board_h)) return fail(SK_EINVAL, "m boards overflow int64 bytes");
  if (device == -1) return skh::render(c, *view, ids, m, out), SK_OK;
  if (device < 0) return fail(SK_EINVAL, "device index out of range");
  for (const void* p : {(const void*)view->pos, (const void*)view->rot, (const void*)view->qpos,
                        (const void*)view->qrot, (const void*)view->qcdage})
    if (((uintptr_t)p) & 15) return fail(SK_EINVAL, "state planes must be 16-byte aligned");
  if (((uintptr_t)view->misc) & 7) return fail(SK_EINVAL, "misc plane must be 8-byte aligned");
  if (((uintptr_t)ids) & 7) return fail(SK_EINVAL, "ids must be 8-byte aligned");
  const hipError_t err = sk_render_launch(c, *view, ids, m, out, (hipStream_t)stream);
  if (err == hipErrorInvalidValue) return fail(SK_EINVAL, "too many boards for one launch");
  HIP_TRY(err);
  return SK_OK;
}

int sk_env_render(sk_env* e, const int64_t* ids, int64_t m, uint8_t* out, void* stream) {
  SK_CHECK_ENV(e);
  return sk_render_states(&e->cfg, e->device, &e->hview, ids, m, out, stream);
}

}  // extern "C"
