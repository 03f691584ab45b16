// CPU check of the fast decisions of the step-only split tick
// (skillshot_learning_amd/csrc/sk_trig.hpp: fast_move_delta, fast_step_delta
// on sincos_fast / sincos_add), compiled for the host with -ffp-contract=off.
// Wherever a fast decision says safe, its integer result must equal the fp64
// expression the exact path evaluates (sincos_bf, the library past its range):
//   move      : rint(p - (sin * speed) * a)         vs  p - (int)rintf(d)
//   fired     : rint(q - sin(rot + l * look) * spd) vs  q - (int)rintf(e), by angle addition
//   in flight : the same step for every later integer q (the carried step),
//               and the step from sincos_fast of the projectile's rotation
// Prints "n=<cases> fallback=<share of random cases sent to the exact path>
// mismatches=<count>" and exits 1 on a mismatch.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../skillshot_learning_amd/csrc/sk_trig.hpp"

static uint64_t rng = 0x9E3779B97F4A7C15ull;
static uint64_t next() {
  rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
  return rng;
}
static double uni(double lo, double hi) { return lo + (hi - lo) * ((next() >> 11) * 0x1p-53); }

static const double kLook = 0.25;
static long n = 0, n_fallback = 0, mismatches = 0;

static float clampf(float a) {
  a = (a >= 1.0f) ? 1.0f : a;
  a = (a <= -1.0f) ? -1.0f : a;
  return a;
}
static double clampd(double a) {
  a = (a >= 1.0) ? 1.0 : a;
  a = (a <= -1.0) ? -1.0 : a;
  return a;
}
static sktrig::SinCos exact(double x) {  // the exact path's value
  bool ok;
  sktrig::SinCos o = sktrig::sincos_bf(x, &ok);
  if (!ok) { o.s = sin(x); o.c = cos(x); }
  return o;
}
static void bad(const char* what, double rot, float a, int p, int speed, double want, long got) {
  if (mismatches++ < 10)
    printf("MISMATCH %s rot=%.17g a=%.9g p=%d speed=%d exact=%.17g fast=%ld\n", what, rot, (double)a, p, speed, want, got);
}

// one case: a player at integer p with rotation rot, move action am, look
// action al; its projectile at integer q.  Returns true when any decision
// went to the exact path.
static bool check(double rot, float am, float al, int p, int q, int pspeed, int qspeed) {
  ++n;
  bool fell = false, ok;
  const sktrig::SinCosF m = sktrig::sincos_fast(rot, &ok);
  const sktrig::SinCos E = exact(rot);
  // the move (Player.py:57-68)
  const sktrig::FastDelta dm = sktrig::fast_move_delta(m, ok, (float)pspeed, clampf(am));
  if (dm.safe) {
    const double speed = clampd((double)am), psp = (double)pspeed;
    const double nxf = rint((double)p - (E.s * psp) * speed), nyf = rint((double)p - (E.c * psp) * speed);
    const long fx = (long)p - (long)(int)rintf(dm.x), fy = (long)p - (long)(int)rintf(dm.y);
    if (!(nxf == (double)fx)) bad("move x", rot, am, p, pspeed, nxf, fx);
    if (!(nyf == (double)fy)) bad("move y", rot, am, p, pspeed, nyf, fy);
  } else {
    fell = true;
  }
  // a projectile fired this tick (Player.py:33-39, :78-89; Projectile.py:38-47)
  const float l = clampf(al);
  const double rn = rot + (double)l * kLook;
  const sktrig::SinCosF u = sktrig::sincos_add(m, l * (float)kLook);
  const sktrig::FastDelta df = sktrig::fast_step_delta(u, ok, (float)qspeed);
  const sktrig::SinCos X = exact(rn);
  const double qsp = (double)qspeed;
  if (df.safe) {
    const int dx = (int)rintf(df.x), dy = (int)rintf(df.y);
    const int at[3] = {q, q - dx, p};  // the launch tick and later ticks of the flight with the carried step
    for (int qq : at) {
      const double ex = rint((double)qq - X.s * qsp), ey = rint((double)qq - X.c * qsp);
      if (!(ex == (double)((long)qq - dx))) bad("fired x", rn, al, qq, qspeed, ex, (long)qq - dx);
      if (!(ey == (double)((long)qq - dy))) bad("fired y", rn, al, qq, qspeed, ey, (long)qq - dy);
    }
  } else {
    fell = true;
  }
  // a projectile in flight whose key missed: the step from sincos_fast(rn)
  bool okq;
  const sktrig::SinCosF g = sktrig::sincos_fast(rn, &okq);
  const sktrig::FastDelta dq = sktrig::fast_step_delta(g, okq, (float)qspeed);
  if (dq.safe) {
    const int dx = (int)rintf(dq.x), dy = (int)rintf(dq.y);
    const double ex = rint((double)q - X.s * qsp), ey = rint((double)q - X.c * qsp);
    if (!(ex == (double)((long)q - dx))) bad("flight x", rn, al, q, qspeed, ex, (long)q - dx);
    if (!(ey == (double)((long)q - dy))) bad("flight y", rn, al, q, qspeed, ey, (long)q - dy);
  } else {
    fell = true;
  }
  return fell;
}

static void both_speeds(double rot, float am, float al, int p, int q) {
  check(rot, am, al, p, q, 3, 5);
  check(rot, am, al, p, q, 5, 3);
}

// The look-step sweep ("look" as the first argument): for each look_speed,
// `count` random (rotation, look action) pairs at projectile speed 5: the
// fired projectile's fp32 decision q - rintf(d) against nearbyint(q - sin(r +
// l * look) * 5) in fp64.  `wrong`: decisions the engine takes from the fp32
// path (look_fits_add(look_speed), the host's gate, and fast_step_delta's
// safe) that differ from the fp64 one: must be 0.  `raw_wrong`: the same
// without the gate, i.e. what sincos_add alone would decide; `max_err`:
// sincos_add's largest error against sinl / cosl.  One line per look_speed.
static int look_sweep(long count) {
  const double looks[] = {0.25, 0.4, 0.78, 0.8, 1.0, 1.5, 3.0};
  long total_wrong = 0;
  for (double look : looks) {
    const bool gate = sktrig::look_fits_add(look);
    long wrong = 0, raw_wrong = 0, safe_n = 0;
    double max_err = 0.0;
    for (long i = 0; i < count; ++i) {
      const double rot = uni(-600.0, 600.0);
      const float l = clampf((float)uni(-1.25, 1.25));
      const int q = (int)(next() % 251);
      bool ok;
      const sktrig::SinCosF m = sktrig::sincos_fast(rot, &ok);
      const double rn = rot + (double)l * look;
      const sktrig::SinCosF u = sktrig::sincos_add(m, l * (float)look);
      const double es = fabs((double)((long double)u.s - sinl((long double)rn)));
      const double ec = fabs((double)((long double)u.c - cosl((long double)rn)));
      max_err = fmax(max_err, fmax(es, ec));
      const sktrig::FastDelta d = sktrig::fast_step_delta(u, ok, 5.0f);
      if (!d.safe) continue;
      ++safe_n;
      const sktrig::SinCos X = exact(rn);
      const bool differs = nearbyint((double)q - X.s * 5.0) != (double)(q - (int)rintf(d.x)) ||
                           nearbyint((double)q - X.c * 5.0) != (double)(q - (int)rintf(d.y));
      raw_wrong += differs;
      wrong += gate && differs;
    }
    printf("look=%g gate=%d n=%ld safe=%ld max_err=%.3e wrong=%ld raw_wrong=%ld\n", look, (int)gate, count, safe_n,
           max_err, wrong, raw_wrong);
    total_wrong += wrong;
  }
  return total_wrong ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && argv[1][0] == 'l') return look_sweep(argc > 2 ? atol(argv[2]) : 4000000);
  const long count = argc > 1 ? atol(argv[1]) : 10000000;
  // random play: game rotations, actions past the clamp, board positions
  for (long i = 0; i < count; ++i) {
    const double rot = (i & 7) ? uni(-600.0, 600.0) : 0.25 * uni(-1.0, 1.0) * (double)(next() % 2000);
    const float am = (float)uni(-1.25, 1.25), al = (float)uni(-1.25, 1.25);
    const int p = (int)(next() % 251), q = (int)(next() % 251);
    const bool sw = (next() & 1) != 0;
    n_fallback += check(rot, am, al, p, q, sw ? 5 : 3, sw ? 3 : 5);
  }
  const long n_random = n;
  // adversarial: deltas at and next to half-integers, the fast range's ends,
  // huge and special rotations, special actions
  const float acts[] = {1.0f, -1.0f, 0.5f, -0.5f, 0.0f, -0.0f, 1.5f, -7.0f, NAN, INFINITY, -INFINITY, 1e-30f};
  for (int speed = 3; speed <= 5; speed += 2)
    for (int k = 1; k < 2 * speed; k += 2)
      for (int turn = -3; turn <= 3; ++turn)
        for (int form = 0; form < 2; ++form) {
          const double h = (double)k / (2.0 * speed);
          const double r0 = (form ? acos(h) : asin(h)) + turn * 2.0 * M_PI;
          const double around[] = {r0, nextafter(r0, 1e9), nextafter(r0, -1e9), r0 + 1e-9, r0 - 1e-9, r0 + 1e-6,
                                   r0 - 1e-6, -r0, M_PI - r0, r0 + M_PI};
          for (double r : around)
            for (float a : acts) {
              both_speeds(r, a, 0.0f, 100, 37);
              both_speeds(r, 1.0f, a, 0, 250);
              both_speeds(r - (double)clampf(a) * kLook, 0.3f, a, 7, 7);  // the fired rotation lands on r
            }
        }
  const double ends[] = {1647099.3291652855, 1647099.0, 1647100.0, 0x1p40, 0x1p52, 1e300, 0.0, -0.0, NAN, INFINITY};
  for (double e : ends)
    for (int sgn = -1; sgn <= 1; sgn += 2)
      for (float a : acts) {
        const double r = sgn * e;
        both_speeds(r, a, a, 125, 125);
        both_speeds(nextafter(r, 1e308), a, 0.7f, 1, 249);
        both_speeds(nextafter(r, -1e308), 0.9f, a, 249, 1);
      }
  const double share = (double)n_fallback / (double)n_random;
  printf("n=%ld fallback=%.3e mismatches=%ld\n", n, share, mismatches);
  return mismatches ? 1 : 0;
}
