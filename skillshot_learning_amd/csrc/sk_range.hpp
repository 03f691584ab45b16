// sk_range.hpp — the integer range tests of the packed split kernel's steady
// tick (k_step_split_multi, sk_engine.hip), host- and device-compilable so
// tests/pair_collision_check.cpp checks these very functions on the CPU.
//
// A closed-interval test lo <= v <= hi costs two signed compares and an AND.
// Where hi >= lo and v - lo does not wrap, one subtraction and one unsigned
// compare decide the same thing: v < lo makes v - lo negative, i.e. above
// every (unsigned)(hi - lo).  The steady loop runs only for a configuration
// the host has checked (cfg_ok below: the boxes fit the board and every
// quantity is far from the int range), so both conditions hold for whatever
// the tick computes, not only for states that fit the packed form.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SKR_HD __host__ __device__ __forceinline__
#else
#define SKR_HD static inline
#endif

namespace skrange {

// every coordinate, size and per-tick step stays below 2^22 in magnitude:
// sums and differences of a few of them cannot wrap
constexpr int kCfgMax = 1 << 20;

// the configurations whose ticks may use the forms below
SKR_HD bool cfg_ok(int W, int H, int psize, int qsize, int pspeed, int qspeed) {
  return (W <= kCfgMax) & (H <= kCfgMax) & (psize >= 0) & (qsize >= 0) & (psize <= W) & (psize <= H) & (qsize <= W) &
         (qsize <= H) & (pspeed >= -kCfgMax) & (pspeed <= kCfgMax) & (qspeed >= -kCfgMax) & (qspeed <= kCfgMax);
}

// 0 <= n && n + size <= extent, as one compare against room = extent - size >= 0
// (player_pos_valid's and Projectile.tick's bounds, one axis)
SKR_HD bool fits_axis(int n, int room) { return (unsigned)n <= (unsigned)room; }

// both axes of a box at (nx, ny) on the board
SKR_HD bool fits_board(int nx, int ny, int room_x, int room_y) {
  return (int)fits_axis(nx, room_x) & (int)fits_axis(ny, room_y);
}

// SkillshotGame.check_collision's corner test of the player box at (px, py)
// against the other player's projectile at (oqx, oqy): hit_test_s without
// its validity flag.  The test is separable: a corner is inside the box
// where its x is (the right or the left one) and its y is (top or bottom).
SKR_HD bool box_hit(int px, int py, int psize, int oqx, int oqy, int qsize) {
  const int dx = oqx - px, dy = oqy - py;
  const bool xl = (unsigned)dx <= (unsigned)psize, xr = (unsigned)(dx + qsize) <= (unsigned)psize;
  const bool yt = (unsigned)dy <= (unsigned)psize, yb = (unsigned)(dy - qsize) <= (unsigned)psize;
  return ((int)xr | (int)xl) & ((int)yt | (int)yb);
}

// One collision test per lane: lane p of a pair evaluates only "my player is
// hit by the partner's projectile" and the pair exchanges the two bits.
// hit_p1 is lane 0's, hit_p2 lane 1's; player 1 is tested first and wins a
// tie (collide_s).  Identical in both lanes.
struct PairHit {
  bool h1, h2;
};
SKR_HD PairHit pair_hit(bool lv, bool hit_p1, bool hit_p2) {
  PairHit r;
  r.h1 = (int)lv & (int)hit_p1;
  r.h2 = (int)lv & (int)!r.h1 & (int)hit_p2;
  return r;
}

}  // namespace skrange
