// sk_bot.hpp — the scripted actors (SK_BOT_*, include/skillshot.h): fixed
// closed-form policies on the game state, host- and device-compilable like
// sk_trig.hpp.  sk_host.cpp (the CPU backend's sk_env_bot_act) and the device
// kernels (k_bot_act, sk_engine.hip; the _bots acting kernels, sk_act32.hpp)
// all evaluate skbot::policy on the same sin / cos primitive (skbot::sincos:
// sktrig::sincos_bf, the library routine past its range), in fp64 with
// contraction off, so both backends give the same floats.
//
// The policy of player p with opponent o on the PRE-tick state, an action
// (move, look) as everywhere else (every seat keeps auto-firing: the step
// does that, not the policy):
//   (s, c) = sin, cos of rot[p];  dx = x[o] - x[p];  dy = y[o] - y[p]
//   side  = s dy - c dx        > 0: the opponent lies on the side a positive look turns to
//   ahead = -(s dx) - c dy     > 0: the opponent lies in front (a move goes by (-s, -c))
//   ahead > 0:  t = side / (ahead look_speed), look = t clamped to [-1, 1]
//   else:       look = -1 if side < 0 else 1   (turn round, by the shorter side)
//   still   (0, 0)
//   random  the caller's two floats (sk_gen_random_actions' for this (game, player) and step)
//   aimer   (0, look)
//   chaser  (1 while the squared distance exceeds (8 player_size)^2, else 0, look)
#pragma once
#include <stdint.h>

#include "../../include/skillshot.h"
#include "sk_trig.hpp"

namespace skbot {

struct Act {
  float move, look;
};

SKT_HD bool kind_ok(int64_t kind) { return kind >= SK_BOT_STILL && kind <= SK_BOT_CHASER; }

// the step's own primitive for a player's old rotation (split_finish's `m`);
// LIB: the caller's library sincos for |x| >= 1.6e6 or a non-finite x
template <typename LIB>
SKT_HD sktrig::SinCos sincos(double rot, LIB lib) {
  bool ok;
  sktrig::SinCos m = sktrig::sincos_bf(rot, &ok);
  if (!ok) m = lib(rot);
  return m;
}

// m = sincos(rot[p]), (dx, dy) = the opponent's position minus the player's;
// r0, r1: the random policy's draw (read for SK_BOT_RANDOM only)
SKT_HD Act policy(int kind, sktrig::SinCos m, int dx, int dy, double look_speed, int player_size, float r0,
                  float r1) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (kind == SK_BOT_RANDOM) return Act{r0, r1};
  if (kind != SK_BOT_AIMER && kind != SK_BOT_CHASER) return Act{0.f, 0.f};
  const double fx = (double)dx, fy = (double)dy;  // ints: exact
  const double side = m.s * fy - m.c * fx;
  const double ahead = -(m.s * fx) - m.c * fy;
  double look;
  if (ahead > 0.0) {
    const double t = side / (ahead * look_speed);
    look = t >= 1.0 ? 1.0 : (t <= -1.0 ? -1.0 : t);
  } else {
    look = side < 0.0 ? -1.0 : 1.0;
  }
  const int64_t d2 = (int64_t)dx * dx + (int64_t)dy * dy, near = 8 * (int64_t)player_size;
  return Act{kind == SK_BOT_CHASER && d2 > near * near ? 1.f : 0.f, (float)look};
}

}  // namespace skbot
