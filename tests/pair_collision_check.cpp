// Host check of csrc/sk_range.hpp, the integer range tests of the packed split
// kernel's steady tick and its one-collision-test-per-lane form, against the
// signed expressions of sk_device.hpp (hit_test_s, collide_s, the bounds of
// player_pos_valid and projectile_tick_s), restated below.
//   pair_collision_check [N random tuples]
// prints key=value fields; exit status 1 on any mismatch or missing case.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../skillshot_learning_amd/csrc/sk_range.hpp"

namespace {

struct Cfg {
  int W, H, psize, qsize;
};

// sk_device.hpp, verbatim but for the qualifiers
bool hit_test_s(const Cfg& c, int px, int py, int oqx, int oqy, int oqvalid) {
  int L = px, R = px + c.psize, T = py, B = py + c.psize;
  int ql = oqx, qr = oqx + c.qsize, qt = oqy, qb = oqy - c.qsize;
  bool xr = (L <= qr) & (qr <= R), xl = (L <= ql) & (ql <= R);
  bool yt = (T <= qt) & (qt <= B), yb = (T <= qb) & (qb <= B);
  return oqvalid && ((xr | xl) & (yt | yb));
}
void collide_s(const Cfg& c, int p1x, int p1y, int q1x, int q1y, int q1v, int p2x, int p2y, int q2x, int q2y, int q2v,
               int& live, int& winner) {
  if (hit_test_s(c, p1x, p1y, q2x, q2y, q2v)) { winner = 1; live = 0; }
  else if (hit_test_s(c, p2x, p2y, q1x, q1y, q1v)) { winner = 2; live = 0; }
}
// the steady tick's signed bounds: the move's and the projectile's
bool move_ok_s(const Cfg& c, int nx, int ny) {
  return (nx >= 0) & (nx <= c.W - c.psize) & (ny >= 0) & (ny <= c.H - c.psize);
}
bool proj_ok_s(const Cfg& c, int nx, int ny) {
  return (nx + c.qsize <= c.W) & (nx >= 0) & (ny + c.qsize <= c.H) & (ny >= 0);
}

uint64_t rng = 0x9E3779B97F4A7C15ull;
uint32_t next() {  // splitmix64
  uint64_t z = (rng += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 32);
}

long mism = 0;
void expect(bool ok, const char* what, long a, long b, long c, long d) {
  if (!ok && mism++ < 10) std::fprintf(stderr, "mismatch %s: %ld %ld %ld %ld\n", what, a, b, c, d);
}

// The interval forms, exhaustively: the collision is separable, so one axis
// at a time over every (player byte, projectile byte) pair, both corners of
// that axis, and then the whole test over every pair on the diagonal axes.
long check_intervals(int psize, int qsize) {
  const Cfg c{250, 250, psize, qsize};
  long n = 0;
  for (int p = 0; p < 256; ++p)
    for (int q = 0; q < 256; ++q, ++n) {
      // x axis alone (y made to overlap: the projectile's top on the box's top), then y alone
      const bool xs = hit_test_s(c, p, 100, q, 100, 1), ys = hit_test_s(c, 100, p, 100, q, 1);
      expect(skrange::box_hit(p, 100, psize, q, 100, qsize) == xs, "x interval", p, q, psize, qsize);
      expect(skrange::box_hit(100, p, psize, 100, q, qsize) == ys, "y interval", p, q, psize, qsize);
      // separable: the signed x and y parts, each from its own pair of intervals
      const int L = p, R = p + psize;
      const bool xr = (L <= q + qsize) & (q + qsize <= R), xl = (L <= q) & (q <= R);
      const bool yt = (L <= q) & (q <= R), yb = (L <= q - qsize) & (q - qsize <= R);
      expect(xs == (xr | xl), "x separable", p, q, psize, qsize);
      expect(ys == (yt | yb), "y separable", p, q, psize, qsize);
      // both axes at once, the other axis running the other way
      expect(skrange::box_hit(p, 255 - p, psize, q, 255 - q, qsize) == hit_test_s(c, p, 255 - p, q, 255 - q, 1),
             "both axes", p, q, psize, qsize);
    }
  return n;
}

// The bounds: a byte position minus every step the steady tick can take.  A
// state that stopped fitting a byte leaves the loop one tick later, so the
// positions run to the board's size; the steps cover +-(speed + 1) for the
// default speeds and far beyond (the forms hold for any int short of a wrap).
long check_bounds(const Cfg& c) {
  long n = 0;
  const int far[] = {-(1 << 20), -70000, -256, 256, 70000, 1 << 20};
  for (int p = -2; p <= c.W + 2; ++p) {
    auto one = [&](int d) {
      const int np = p - d;
      for (int o = 0; o < 3; ++o) {  // the other axis inside, at its upper bound, one past it
        const int om = c.H - c.psize + (o - 1), oq = c.H - c.qsize + (o - 1);
        expect(skrange::fits_board(np, om, c.W - c.psize, c.H - c.psize) == move_ok_s(c, np, om), "move x", p, d, o, 0);
        expect(skrange::fits_board(om, np, c.W - c.psize, c.H - c.psize) == move_ok_s(c, om, np), "move y", p, d, o, 0);
        expect(skrange::fits_board(np, oq, c.W - c.qsize, c.H - c.qsize) == proj_ok_s(c, np, oq), "proj x", p, d, o, 0);
        expect(skrange::fits_board(oq, np, c.W - c.qsize, c.H - c.qsize) == proj_ok_s(c, oq, np), "proj y", p, d, o, 0);
        n += 4;
      }
    };
    for (int d = -300; d <= 300; ++d) one(d);
    for (int d : far) one(d);
  }
  return n;
}

}  // namespace

int main(int argc, char** argv) {
  const long N = argc > 1 ? std::atol(argv[1]) : 10000000;
  long cases = 0;
  const int sizes[][2] = {{5, 3}, {1, 1}, {255, 255}, {1, 255}, {255, 1}};
  for (auto& s : sizes) cases += check_intervals(s[0], s[1]);
  cases += check_bounds(Cfg{250, 250, 5, 3});
  cases += check_bounds(Cfg{250, 250, 1, 1});
  cases += check_bounds(Cfg{255, 255, 255, 255});
  cases += check_bounds(Cfg{300, 7, 7, 2});
  if (!skrange::cfg_ok(250, 250, 5, 3, 3, 5) || skrange::cfg_ok(4, 250, 5, 3, 3, 5) || skrange::cfg_ok(250, 2, 5, 3, 3, 5) ||
      skrange::cfg_ok(1 << 21, 250, 5, 3, 3, 5) || skrange::cfg_ok(250, 250, 5, 3, 1 << 21, 5))
    expect(false, "cfg_ok", 0, 0, 0, 0);

  // random full tuples, oriented as lane 0 and lane 1 hold them, combined as the kernel does
  const Cfg c{250, 250, 5, 3};
  long h1_only = 0, h2_only = 0, both = 0, neither = 0, invalid_overlap = 0, dead_hit = 0;
  for (long i = 0; i < N; ++i) {
    const uint32_t a = next(), b = next(), f = next();
    int px[2], py[2], qx[2], qy[2], qv[2];
    px[0] = a & 0xff; py[0] = (a >> 8) & 0xff; px[1] = (a >> 16) & 0xff; py[1] = a >> 24;
    qx[0] = b & 0xff; qy[0] = (b >> 8) & 0xff; qx[1] = (b >> 16) & 0xff; qy[1] = b >> 24;
    // most projectiles near the player they threaten, so hits are common
    if (f & 0x100) { qx[1] = (px[0] + (int)((f >> 9) % 13) - 5) & 0xff; qy[1] = (py[0] + (int)((f >> 13) % 13) - 3) & 0xff; }
    if (f & 0x20000) { qx[0] = (px[1] + (int)((f >> 18) % 13) - 5) & 0xff; qy[0] = (py[1] + (int)((f >> 22) % 13) - 3) & 0xff; }
    qv[0] = (f & 3) != 0; qv[1] = (f & 12) != 0;
    const int live0 = (f & 0xf0) != 0, winner0 = (int)(f >> 30);
    int live = live0, winner = winner0;
    if (live) collide_s(c, px[0], py[0], qx[0], qy[0], qv[0], px[1], py[1], qx[1], qy[1], qv[1], live, winner);
    // lane p: its own player against the partner's projectile (pair_swap of qx, qy, qvalid)
    bool mine[2];
    for (int p = 0; p < 2; ++p)
      mine[p] = (qv[p ^ 1] != 0) & skrange::box_hit(px[p], py[p], c.psize, qx[p ^ 1], qy[p ^ 1], c.qsize);
    for (int p = 0; p < 2; ++p) {  // each lane combines its bit with the partner's (one more pair_swap)
      const bool m = mine[p], t = mine[p ^ 1];
      const skrange::PairHit h = skrange::pair_hit(live0 != 0, p ? t : m, p ? m : t);
      const int w = h.h1 ? 1 : (h.h2 ? 2 : winner0), lv = (h.h1 | h.h2) ? 0 : live0;
      expect(w == winner && lv == live, "pair", i, p, w, winner);
    }
    const bool g1 = skrange::box_hit(px[0], py[0], c.psize, qx[1], qy[1], c.qsize);
    const bool g2 = skrange::box_hit(px[1], py[1], c.psize, qx[0], qy[0], c.qsize);
    if (live0) {
      h1_only += mine[0] && !mine[1];
      h2_only += !mine[0] && mine[1];
      both += mine[0] && mine[1];
      neither += !mine[0] && !mine[1];
      invalid_overlap += (g1 && !qv[1]) || (g2 && !qv[0]);
    } else {
      dead_hit += mine[0] || mine[1];
    }
  }
  const bool covered = h1_only && h2_only && both && neither && invalid_overlap && dead_hit;
  std::printf("n=%ld exhaustive=%ld mismatches=%ld h1_only=%ld h2_only=%ld both=%ld neither=%ld invalid_overlap=%ld dead_hit=%ld\n",
              N, cases, mism, h1_only, h2_only, both, neither, invalid_overlap, dead_hit);
  return (mism == 0 && covered) ? 0 : 1;
}
