// sk_multi_plan.hpp — which multi-tick kernel a launch runs (sk_env_step_multi,
// sk_env_step_multi_obs): the SK_MULTI_* knobs, the size / tick thresholds and
// plan_multi, a pure function from a launch's sizes and knobs to the
// instantiation of k_step_multi / k_step_split_multi (sk_multi.hpp) and its
// runtime arguments.  Host-only and free of HIP, so tests/test_multi_plan_cpu.py
// pins every decision without a device (skdiag_multi_plan, sk_engine.hip)
// against a table recorded from the logic this header replaced
// (tests/golden/multi_plan.npz).  step_multi (sk_engine.hip) fills a
// MultiPlanIn, plans, and hands the plan to launch_plan.
#pragma once
#include <stdint.h>

#include <cstdlib>

namespace skplan {

// the SK_MULTI_* environment knobs, read once per handle (make_env)
struct MultiKnobs {
  // k_step_multi state port: 1 write-through (default: the contract bytes leave L2 every tick), 0 plain
  // (SK_MULTI_POLICY)
  int policy = 1;
  // k_step_multi geometry: -1 auto, 0 lane per game, 1 player per lane (SK_MULTI_SPLIT)
  int split = -1;
  int early = -1;     // k_step_multi: the restart draw under the loads, -1 (default: on) / 0 / 1 (SK_MULTI_EARLY)
  int block = -1;     // workgroup lanes (SK_MULTI_BLOCK): split geometry -1 auto, 64 or 512; lane per game 64 or 256
  int stagger = 0;    // waves 4-7 of a 512-lane workgroup start this x 512 cycles late (SK_MULTI_STAGGER)
  int prefetch = -1;  // action-slab prefetch wave, ticks ahead (SK_MULTI_PREFETCH; 0 off, -1 auto): k_step_multi
                      // (64-lane, 88-B form) and k_step_split_multi
  // the packed resident form between ticks (k_step_multi, step-only
  // k_step_split_multi): -1 auto (above one wave per SIMD), 1 / 0 force
  // (SK_MULTI_PACK)
  int pack = -1;
  // the step-only k_step_split_multi on fp32 trig with the exact fallback
  // (split_tick_carry's FAST form): -1 auto (the packed form's sizes in
  // launches from kFastSplitMinTicks ticks), 1 / 0 force (SK_MULTI_FAST)
  int fast = -1;
};

inline MultiKnobs multi_knobs_from_env() {
  static constexpr struct {
    const char* name;
    int MultiKnobs::*field;
  } kKnobs[] = {{"SK_MULTI_POLICY", &MultiKnobs::policy},     {"SK_MULTI_SPLIT", &MultiKnobs::split},
                {"SK_MULTI_EARLY", &MultiKnobs::early},       {"SK_MULTI_BLOCK", &MultiKnobs::block},
                {"SK_MULTI_STAGGER", &MultiKnobs::stagger},   {"SK_MULTI_PREFETCH", &MultiKnobs::prefetch},
                {"SK_MULTI_PACK", &MultiKnobs::pack},         {"SK_MULTI_FAST", &MultiKnobs::fast}};
  MultiKnobs k;
  for (const auto& kn : kKnobs)
    if (const char* v = std::getenv(kn.name)) k.*kn.field = std::atoi(v);
  return k;
}

// k_step_multi's packed resident form above this many games (one wave per
// SIMD on 1,024 SIMDs).  By default the lane-per-game kernel runs only above
// kSplitPackMaxEnvs; this bound is what SK_MULTI_SPLIT=0 leaves in force
constexpr int64_t kPackMinEnvs = 65536;
// k_step_multi: two lanes per game with the 88-B form up to this many games.
// Write-through port, 400 ticks per launch: 8,192 games 1.59 vs 1.85 us per
// tick, 32,768 1.80 vs 2.02, but 65,536 2.59 vs 2.36
// (profiles/r03c_multi_split_sweep.jsonl); these sizes run the PACK = false
// instantiations, which the packed one left as they were
constexpr int64_t kSplitMultiMaxEnvs = 32768;
// k_step_split_multi's packed instantiation (two or three waves per SIMD over
// 48 B per game and tick, 64-lane workgroups) for this range of games.
// Write-through port, 400 ticks per launch, us per tick against the default
// before it (k_step_multi: the 88-B form up to 65,536 games, packed above):
// 40,960 games 1.73-1.75 vs 1.79-1.84, 49,152 1.75-1.76 vs 1.81-1.82, 57,344
// 1.78-1.79 vs 2.00, 65,536 1.80-1.81 vs 2.02-2.09, 81,920 2.19-2.21 vs
// 2.87-2.89, 98,304 2.23-2.26 vs 2.91-2.95; but 114,688 3.25-3.31 vs
// 3.06-3.08 and 131,072 3.33-3.35 vs 3.07-3.13: from there k_step_multi's
// packed form (profiles/r08_split_pack_boundary.jsonl)
constexpr int64_t kSplitPackMinEnvs = 40960;
constexpr int64_t kSplitPackMaxEnvs = 98304;
// k_step_split_multi's fp32-trig tick (FAST) where several waves share a SIMD
// and the launch is long: 267 against 321 VALU per wave and tick.  Write-
// through port, us per tick, fast against the fp64 carry at 400 / 100 / 20
// ticks per launch: 40,960 games 1.64-1.65 vs 1.69-1.70 / 1.68-1.70 vs 1.72 /
// 1.92 vs 1.87-1.88; 65,536 1.71 vs 1.75-1.76 / 1.75-1.76 vs 1.78-1.79 /
// 2.09 vs 1.96-1.97; 98,304 2.04-2.06 vs 2.17-2.22 / 2.09-2.11 vs 2.21-2.22 /
// 2.43-2.44 either way.  One wave per SIMD loses at every launch length
// (8,192: 1.27 vs 1.19 / 1.31 vs 1.21 / 1.48 vs 1.33; 32,768: 1.40 vs 1.35 /
// 1.45 vs 1.40 / 1.73 vs 1.53): there the tick is a latency chain and the
// fp64 carry runs under the loads for nothing
// (profiles/r09_split_fast_sweep.jsonl)
constexpr int kFastSplitMinTicks = 100;
// 512-lane workgroups from 65,536 games for the 88-B form; the packed form
// stays on 64-lane ones (65,536 games 1.80 vs 1.78-1.79 us per tick, but
// 98,304, 384 workgroups of 512 on 256 CUs, 2.22 vs 3.31;
// profiles/r08_split_pack_first_sweep.jsonl)
constexpr int64_t kSplitWideMinLanes = 512 * 256;
// the action-slab prefetch wave: SK_MULTI_PREFETCH, else, at 400 ticks
// per launch: the full contract 4 ticks ahead on 512-lane workgroups
// (65,536 games 4.35 -> 3.48-3.52 us per tick) and 1 on 64-lane ones
// (32,768 2.71 -> 2.59, 8,192 2.25 -> 2.24-2.25; profiles/
// r04ar_prefetch_*_sweep.jsonl, r04as_prefetch_obs64_sweep.jsonl).  The
// step-only tick runs split_tick_carry (round 6), which loads the slab a
// tick ahead itself: no prefetch wave (8,192 games 1.58 -> 1.20 us per
// tick, 32,768 1.68 -> 1.46; profiles/r06x_split_carry_sweep.jsonl).  The
// full contract on split_tick_carry: no prefetch wave on 64-lane
// workgroups (8,192 2.23 -> 1.96, 32,768 2.55 -> 2.29), and still 4 ticks
// ahead on 512-lane ones (65,536 3.38-3.57 -> 3.20-3.39; profiles/
// r06aa_obs_carry_sweep.jsonl, r06ab_obs_carry_pf_sweep.jsonl)
// With the step-only carried tick the prefetch wave still pays at 32,768
// games (2 ticks ahead: 1.46 -> 1.35 us at 400 ticks per launch, 1.64 ->
// 1.54 at 20), not at 8,192 (1.20 either way) nor 65,536
// (profiles/r06ad_split_carry_pf_sweep.jsonl)
constexpr int64_t kSplitPrefetchAboveEnvs = 8192;

// The packed split kernel's steady loop addresses the action ring and the
// done / winner rows with 32-bit byte offsets off a buffer resource: every
// slab of the ring (ring_slabs x 16 n bytes) and every output row
// (out_slabs x out_stride, plus a row's n bytes) must lie below 4 GiB, and
// both ring positions must fit an int.  A launch outside these bounds keeps
// the generic tick's 64-bit addressing for all of its ticks (MultiArgs::
// steady32 = 0): same results.
inline bool split_steady_fits32(int64_t n, int64_t ring_slabs, int64_t out_slabs, int64_t out_stride) {
  const uint64_t lim = 0xffffffffull;
  if (n <= 0 || ring_slabs <= 0 || out_slabs <= 0 || out_stride < 0) return false;
  if ((uint64_t)n > lim / 16u || (uint64_t)ring_slabs > lim / (16u * (uint64_t)n)) return false;
  if ((uint64_t)out_slabs > 0x7fffffffull) return false;
  if (out_stride > 0 && (uint64_t)out_slabs > (lim - (uint64_t)n) / (uint64_t)out_stride) return false;
  return true;
}

// everything the decision reads
struct MultiPlanIn {
  int64_t n;
  int n_ticks;
  bool full;          // sk_env_step_multi_obs: the obs / reward epilogue
  bool restart_fits;  // the configuration's restart positions fit a byte (the packed form needs it)
  bool pack_allowed;  // false: the pack buffer is missing and the stream is capturing (no allocation there)
  bool planes_fit32;  // the six state planes lie within 4 GiB of the lowest (the write-through port's one resource)
  bool steady_ok;     // split_steady_fits32 && skrange::cfg_ok && skrange::admit_cfg
  MultiKnobs knobs;
};

// the instantiation launched and its runtime arguments, in effective values
struct MultiPlan {
  bool split;     // k_step_split_multi (two lanes per game), else k_step_multi (one)
  int pol;        // state port: 1 write-through, 0 plain (also where the planes do not fit 32-bit offsets)
  int blk;        // workgroup lanes that tick: 64 / 512 (split), 64 / 256 (lane per game)
  bool obs;       // the full contract's epilogue (split only)
  int pf;         // prefetch / feed wave, ticks ahead: 0 (none), 1, 2 or 4
  bool pack;      // the packed resident form between ticks
  bool fast;      // split_tick_carry's fp32-trig form (split, step-only)
  int stagger;    // k_step_split_multi's argument (0 unless 512-lane workgroups)
  int early;      // k_step_multi's argument (0 in the split geometry)
  int steady32;   // MultiArgs::steady32
  unsigned grid;  // workgroups
  int block_threads;  // blk, + 64 with a prefetch or feed wave
};

// the launchers' own mapping of a requested distance to an instantiated one
inline int pf_instantiated(int pf) { return pf == 1 ? 1 : pf == 2 ? 2 : pf > 2 ? 4 : 0; }

inline MultiPlan plan_multi(const MultiPlanIn& in) {
  const MultiKnobs& k = in.knobs;
  const int64_t n = in.n;
  MultiPlan p{};
  p.steady32 = in.steady_ok ? 1 : 0;
  // the packed resident form pays where the tick is bandwidth-bound (two or
  // more waves per SIMD: 131,072 games 3.33 vs 4.03 us per tick, 262,144 6.4
  // vs 7.7); at one wave per SIMD the tick is a latency chain and the
  // pack / unpack work lengthens it (65,536: 2.51 vs 2.38; 32,768: 2.43 vs
  // 2.04; profiles/r03pk2_multi_pack_sweep.jsonl)
  // In the split geometry 65,536 games already are two waves per SIMD, and
  // there the packed form is what lifts the tick off the fabric's bandwidth
  // (kSplitPackMinEnvs .. kSplitPackMaxEnvs).  Both kernels take the pack
  // decision before the restart (the early store), so the packed form needs a
  // configuration whose restart positions fit a byte.
  const bool sp_range = n >= kSplitPackMinEnvs && n <= kSplitPackMaxEnvs && in.restart_fits;
  const bool pack_avail =
      in.pack_allowed && !in.full && in.n_ticks > 1 && k.pack != 0 && (uint64_t)n * 48u <= 0xffffffffull;
  // geometry: one lane per game (k_step_multi) or two (k_step_split_multi);
  // SK_MULTI_SPLIT = 0 / 1 forces one, else auto (kSplitMultiMaxEnvs, and the
  // packed split kernel's range where the packed form is to be had)
  // (the full contract always runs the split geometry: a lane per player
  // computes that player's observation, as k_step_split does)
  p.split = in.full || (k.split >= 0 ? k.split != 0 : (n <= kSplitMultiMaxEnvs || (pack_avail && sp_range)));
  p.pack = pack_avail && in.restart_fits && (k.pack > 0 || (p.split ? sp_range : n > kPackMinEnvs));
  // planes farther apart than one 32-bit buffer offset (a caller's own
  // allocations; VecSkillshotGame and sk_env_create use one block): the
  // plain port, same results
  p.pol = k.policy == 1 && in.planes_fit32 ? 1 : 0;
  if (p.split) {
    const int64_t lanes = 2 * n;
    const bool wide = k.block == 512 || (k.block < 0 && !p.pack && lanes >= kSplitWideMinLanes);
    p.blk = wide ? 512 : 64;
    p.grid = (unsigned)((lanes + p.blk - 1) / p.blk);
    p.obs = in.full;
    const int pf = in.n_ticks < 2                             ? 0
                   : k.prefetch >= 0                          ? k.prefetch
                   : in.full                                  ? (wide ? 4 : 0)
                   : (n > kSplitPrefetchAboveEnvs && !wide) ? 2
                                                              : 0;
    // the packed form has no prefetch wave, nor has the plain port
    p.pf = p.pack || p.pol != 1 ? 0 : pf_instantiated(pf);
    p.stagger = wide ? k.stagger : 0;
    // the fp32-trig tick (step-only): SK_MULTI_FAST = 0 / 1 forces, else auto:
    // the packed form's sizes (kSplitPackMinEnvs) in launches from
    // kFastSplitMinTicks ticks
    p.fast = !in.full &&
             (k.fast >= 0 ? k.fast != 0 : (p.pack && n >= kSplitPackMinEnvs && in.n_ticks >= kFastSplitMinTicks));
  } else {
    // the restart draw under the loads (k_step's early draw): off in round 3
    // (65,536 games 2.73 vs 2.81 us per tick at 20 ticks per launch;
    // profiles/r03i_multi_fast_early_sweep.jsonl); with round 6's tick the
    // wait it hides under has room, and the draw leaves the restarting waves'
    // chain: on by default (SK_MULTI_EARLY=0 off), the driver's 20-tick
    // region 2.53-2.55 -> 2.51-2.54 us, 20-tick launches back to back 2.35
    // -> 2.30-2.33 (profiles/r06af_multi_early_ab.jsonl)
    p.early = k.early != 0;
    // workgroup: four waves (default; SK_MULTI_BLOCK=64: one).  A quarter of
    // the workgroups to dispatch, one wave per SIMD either way.  Round 3 had
    // 64 lanes ahead by ~0.6 % with the 88-B form (profiles/
    // r03mb_multi_block_ab.jsonl, r03mb2_multi_block_early_ab.jsonl); with the
    // round-6 tick (early stores, the slab a tick ahead) 256 lanes take the
    // driver's 20-tick launch from 2.52-2.56 to 2.48-2.50 us per tick (median
    // of 30 regions, three passes; profiles/r06p_k20_block_ab.jsonl)
    const bool four = k.block == 256 || (k.block < 0 && k.prefetch <= 0);
    p.blk = four ? 256 : 64;
    p.grid = (unsigned)((n + p.blk - 1) / p.blk);
    // the feed wave only on request (auto: none), and only for the 88-B form
    // on 64-lane workgroups through the write-through port: 65,536 games
    // 2.36 vs 2.33-2.39 us per tick at PF 1-4 and slower at 20 ticks per
    // launch, where actions held in cache (an 8-slab ring) give 2.0
    // (profiles/r04aq_prefetch_sweep.jsonl, r04at_prefetch_ring_sweep.jsonl)
    p.pf = (!four && !p.pack && p.pol == 1 && in.n_ticks > 1 && n % 64 == 0 && k.prefetch > 0)
               ? pf_instantiated(k.prefetch)
               : 0;
  }
  p.block_threads = p.blk + (p.pf > 0 ? 64 : 0);
  return p;
}

}  // namespace skplan
