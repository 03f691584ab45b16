// sk_range.hpp — the integer range tests of the packed split kernel's steady
// tick (k_step_split_multi, sk_multi.hpp), host- and device-compilable so
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

// ---- the packed form's ranges (pack_pos / pack_cah, sk_multi.hpp): a byte
// per coordinate, a signed byte of cooldown, a byte of age, 16 bits of ticks
SKR_HD bool pack_fits_player(int px, int py, int qx, int qy, int cd, int age, int qv) {
  return ((unsigned)px < 256u) & ((unsigned)py < 256u) & ((unsigned)qx < 256u) & ((unsigned)qy < 256u) &
         (cd >= -128) & (cd <= 127) & ((unsigned)age < 256u) & ((unsigned)qv < 2u);
}
SKR_HD bool pack_fits_game(int ticks, int live, int winner) {
  return ((unsigned)ticks < 65536u) & ((unsigned)live < 2u) & ((unsigned)winner < 4u);
}

// ---- admission to the steady loop for the rest of a launch.  A state that
// fits the packed form now keeps fitting it for `left` more ticks under
// split_tick_carry's integer rules if the configuration passes admit_cfg and
// the post-tick state admit_player / admit_game:
//   positions  change only to one that passed fits_board against a room of at
//              most 255, to the player's (a fired projectile), or to a restart
//              position (the host's restart_fits);
//   qcd        is <= 0 (fires: becomes cdmax, or cdmax - 1 in a live game) or
//              counts down by one per live tick: within [-128, 127] at entry,
//              it stays within [min(entry, -1), max(entry, cdmax)];
//   qage       grows by one per live tick while qcd counts down and restarts
//              from 0 at a fire, so qage + max(qcd, 0) never grows except to
//              max(cdmax, 1) at a fire: at most 255 at entry, at most 255 later;
//   ticks      grows by at most one per tick, or restarts from 0;
//   qvalid, live, winner only take the values the tick writes (0 / 1, 0 / 1,
//              0 .. 2).
// tests/steady_admit_check.cpp runs the recurrence over every entry.
// (admit_cfg: for a configuration that passed cfg_ok, whose differences cannot wrap)
SKR_HD bool admit_cfg(int W, int H, int psize, int qsize, int cdmax) {
  return (cdmax >= 0) & (cdmax <= 127) & (W - psize <= 255) & (H - psize <= 255) & (W - qsize <= 255) &
         (H - qsize <= 255);
}
SKR_HD bool admit_player(int px, int py, int qx, int qy, int cd, int age, int qv) {
  // (unsigned sums: no wrap to undefined behaviour for a state that does not fit, which the first term rejects)
  return (int)pack_fits_player(px, py, qx, qy, cd, age, qv) & (int)((unsigned)age + (unsigned)(cd > 0 ? cd : 0) <= 255u);
}
// left: the ticks of the launch after this one
SKR_HD bool admit_game(int ticks, int live, int winner, int left) {
  return (int)pack_fits_game(ticks, live, winner) & (int)((unsigned)left <= 65535u) &
         (int)((unsigned)ticks + ((unsigned)left & 0xffffu) <= 65535u);
}

}  // namespace skrange
