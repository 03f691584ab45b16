// sk_stats.hpp — the match statistics (SK_STAT_*, include/skillshot.h): what
// one seat did over the ticks its game lived, tallied in int32.  Host- and
// device-compilable like sk_bot.hpp: sk_host.cpp (the CPU backend's
// sk_env_stats_tick) and the device kernels (k_stats_tick, sk_engine.hip; the
// _stats league kernel, sk_act32.hpp) all run skstat::tick, in fp64 with
// contraction off and on skbot::sincos, so both backends and both paths count
// the same ticks.
//
// One call updates the accumulators of player p with opponent o from one
// PRE-tick state of a game that lives at that tick (live and ticks <
// tick_limit: the caller's test).  (dx, dy) = pos[o] - pos[p], cheb =
// max(|dx|, |dy|), side and ahead as skbot::policy's:
//   shots       +1 if cooldown[p] <= 0            (the seat fires this tick)
//   in_flight   +1 if p's projectile is valid
//   on_target   +1 if ahead > 0 and |side| <= player_size
//   under_fire  +1 if o's projectile is valid and within 2 player_size
//               (Chebyshev) of p's position
//   at_wall     +1 if a full-speed move along an axis would leave the board
//   path        += |x - x_prev| + |y - y_prev| (0 at the first lived tick)
//   dist_sum    += cheb
//   closest     = min(closest, cheb), from INT32_MAX
// x_prev == kNoPrev marks "no lived tick yet".
#pragma once
#include <stdint.h>

#include "../../include/skillshot.h"
#include "sk_bot.hpp"
#include "sk_trig.hpp"

namespace skstat {

constexpr int32_t kNoPrev = INT32_MIN;  // x_prev before the first lived tick
constexpr int32_t kFar = INT32_MAX;     // closest of a game that played no tick

// dist_sum grows by at most max(W, H) per tick (and path, between two ticks of
// one game, by at most 2 player_speed): tick_limit max(W, H) must fit int32
SKT_HD bool fits(int64_t tick_limit, int64_t board_w, int64_t board_h) {
  const int64_t m = board_w > board_h ? board_w : board_h;
  return tick_limit >= 0 && m >= 0 && (m == 0 || tick_limit <= (int64_t)INT32_MAX / m);
}

SKT_HD int iabs(int v) { return v < 0 ? -v : v; }

// s: the eight accumulators; (xp, yp): the previous lived tick's position;
// m = skbot::sincos(rot[p]); (x, y) / (ox, oy): p's / o's position; cd: p's
// cooldown; own_valid / opp_valid: the projectiles' flags; (oqx, oqy): o's
// projectile
SKT_HD void tick(int32_t (&s)[SK_N_STATS], int32_t& xp, int32_t& yp, sktrig::SinCos m, int x, int y, int ox, int oy,
                 int cd, bool own_valid, bool opp_valid, int oqx, int oqy, int player_size, int player_speed,
                 int board_w, int board_h) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int dx = ox - x, dy = oy - y;
  const int cheb = iabs(dx) > iabs(dy) ? iabs(dx) : iabs(dy);
  const double fx = (double)dx, fy = (double)dy;  // ints: exact
  const double side = m.s * fy - m.c * fx;
  const double ahead = -(m.s * fx) - m.c * fy;
  const int fdx = iabs(oqx - x), fdy = iabs(oqy - y);
  const bool first = xp == kNoPrev;
  s[SK_STAT_SHOTS] += cd <= 0 ? 1 : 0;
  s[SK_STAT_IN_FLIGHT] += own_valid ? 1 : 0;
  s[SK_STAT_ON_TARGET] += (ahead > 0.0 && __builtin_fabs(side) <= (double)player_size) ? 1 : 0;
  s[SK_STAT_UNDER_FIRE] += (opp_valid && (fdx > fdy ? fdx : fdy) <= 2 * player_size) ? 1 : 0;
  s[SK_STAT_AT_WALL] += (x < player_speed || y < player_speed || x + player_size + player_speed > board_w ||
                         y + player_size + player_speed > board_h)
                            ? 1
                            : 0;
  s[SK_STAT_PATH] += first ? 0 : iabs(x - xp) + iabs(y - yp);
  s[SK_STAT_DIST_SUM] += cheb;
  s[SK_STAT_CLOSEST] = cheb < s[SK_STAT_CLOSEST] ? cheb : s[SK_STAT_CLOSEST];
  xp = x;
  yp = y;
}

}  // namespace skstat
