// Host check of the packed split kernel's launch-long admission to its steady
// loop (csrc/sk_range.hpp: admit_cfg, admit_player, admit_game, and the
// pack_fits_* tests they imply), compiled for the CPU.  The tick's integer
// rules are modelled here as split_tick_carry states them (sk_multi.hpp):
//
//   f = qcd <= 0;  if (f) { qcd = cdmax; qage = 0; qvalid = 1; }
//   ticks += lv;  qcd -= lv;  qage += lv;          lv: the game is live
//   a live game may die in any tick (lv = 0 from the next one);
//   a restart sets qcd = qage = ticks = 0, live = 1.
//
// 1. One-step induction, exhaustive: for every cdmax in [0, 127], every
//    (qcd, qage) in [-128, 127] x [0, 255] that admit_player admits and both
//    values of lv, the next state is admitted again (so it fits the packed
//    form): covers a game dying at any tick, or never, over any number of
//    ticks.  The same for admit_game over (ticks, left), with the restart.
// 2. The recurrence run out: every entry pair, cdmax in {0, 1, 15, 126, 127},
//    480 live ticks, and at each of them the branch "the game died here" run
//    to its fixed point: no admitted entry ever leaves the form; rejected
//    entries exist that do leave it ((5, 251) at its fifth tick) and admitted
//    ones that reach qage = 255 exactly ((5, 250) among them).
// 3. admit_cfg at its bounds.
//
// Prints key=value pairs; exit status 1 on any violation.
#include <cstdio>
#include <cstdlib>

#include "../skillshot_learning_amd/csrc/sk_range.hpp"

namespace {

struct P {
  int qcd, qage, qv;
};
// one tick of a player's projectile clock
P tick(P s, int cdmax, int lv) {
  if (s.qcd <= 0) {
    s.qcd = cdmax;
    s.qage = 0;
    s.qv = 1;
  }
  s.qcd -= lv;
  s.qage += lv;
  return s;
}
bool fits(const P& s) { return skrange::pack_fits_player(0, 0, 0, 0, s.qcd, s.qage, s.qv); }
bool admitted(const P& s) { return skrange::admit_player(0, 0, 0, 0, s.qcd, s.qage, s.qv); }

}  // namespace

int main() {
  long long violations = 0, induction = 0, game_steps = 0;
  // ---- 1. one-step induction
  for (int cdmax = 0; cdmax <= 127; ++cdmax)
    for (int qcd = -128; qcd <= 127; ++qcd)
      for (int qage = 0; qage <= 255; ++qage)
        for (int qv = 0; qv <= 1; ++qv) {
          const P s{qcd, qage, qv};
          if (!fits(s)) ++violations;  // the whole entry range fits the form
          if (!admitted(s)) continue;
          for (int lv = 0; lv <= 1; ++lv) {
            const P n = tick(s, cdmax, lv);
            ++induction;
            if (!admitted(n) || !fits(n)) ++violations;
          }
        }
  if (!admitted(P{0, 0, 0})) ++violations;  // a restart
  // the game's half: ticks grows by at most one while `left` falls by one
  const int lefts[] = {0, 1, 2, 10, 399, 400, 65534, 65535};
  for (int ticks = 0; ticks <= 65535; ++ticks)
    for (int left : lefts)
      for (int live = 0; live <= 1; ++live) {
        if (!skrange::admit_game(ticks, live, 0, left)) continue;
        if (ticks + left > 65535) ++violations;
        if (left == 0) continue;
        for (int lv = 0; lv <= live; ++lv) {
          ++game_steps;
          if (!skrange::admit_game(ticks + lv, live, lv ? 2 : 0, left - 1)) ++violations;
          if (!skrange::pack_fits_game(ticks + lv, live, 2)) ++violations;
        }
        if (!skrange::admit_game(0, 1, 0, left - 1)) ++violations;  // restarted
      }
  long long game_bound = 0;
  game_bound += skrange::admit_game(65535 - 12, 1, 0, 12) && !skrange::admit_game(65536 - 12, 1, 0, 12);
  game_bound += !skrange::admit_game(0, 1, 0, 65536) && !skrange::admit_game(0, 1, 0, -1) &&
                !skrange::admit_game(-1, 1, 0, 0) && !skrange::admit_game(0, 2, 0, 0) && !skrange::admit_game(0, 1, 4, 0);
  // ---- 2. the recurrence run out
  const int cds[] = {0, 1, 15, 126, 127};
  const int T = 480;
  long long runs = 0, admitted_entries = 0, reach_255 = 0, rejected_leave = 0;
  bool saw_5_250 = false, saw_5_251 = false;
  for (int cdmax : cds)
    for (int qcd = -128; qcd <= 127; ++qcd)
      for (int qage = 0; qage <= 255; ++qage) {
        const P e{qcd, qage, 1};
        const bool adm = admitted(e);
        admitted_entries += adm;
        bool left_form = false;
        int top = qage, left_at = -1;
        P s = e;
        for (int t = 0; t < T; ++t) {
          // the game died before this tick: its clock runs with lv = 0
          P d = tick(s, cdmax, 0);
          const P d2 = tick(d, cdmax, 0), d3 = tick(d2, cdmax, 0);
          if (!fits(d) || !fits(d2)) left_form = true;
          if (d3.qcd != d2.qcd || d3.qage != d2.qage) ++violations;  // a fixed point from there
          s = tick(s, cdmax, 1);
          if (!fits(s) && !left_form) {
            left_form = true;
            left_at = t;
          }
          if (s.qage > top) top = s.qage;
        }
        ++runs;
        if (adm && left_form) ++violations;
        if (adm && top == 255) ++reach_255;
        if (!adm && left_form) ++rejected_leave;
        if (cdmax == 15 && qcd == 5 && qage == 250) saw_5_250 = adm && top == 255 && !left_form;
        if (cdmax == 15 && qcd == 5 && qage == 251) saw_5_251 = !adm && left_form && left_at == 4;  // its fifth tick
      }
  if (!saw_5_250 || !saw_5_251) ++violations;
  // ---- 3. the configuration's bounds
  long long cfg = 0;
  cfg += skrange::admit_cfg(250, 250, 5, 3, 15);
  cfg += skrange::admit_cfg(260, 260, 5, 5, 127) && !skrange::admit_cfg(261, 260, 5, 5, 127) &&
         !skrange::admit_cfg(260, 261, 5, 5, 127) && !skrange::admit_cfg(260, 260, 5, 4, 127) &&
         !skrange::admit_cfg(260, 260, 4, 5, 127);
  cfg += skrange::admit_cfg(250, 250, 5, 3, 0) && !skrange::admit_cfg(250, 250, 5, 3, -1) &&
         !skrange::admit_cfg(250, 250, 5, 3, 128);
  if (cfg != 3 || game_bound != 2) ++violations;
  std::printf("violations=%lld induction=%lld game_steps=%lld runs=%lld admitted=%lld reach_255=%lld rejected_leave=%lld\n",
              violations, induction, game_steps, runs, admitted_entries, reach_255, rejected_leave);
  return violations ? 1 : 0;
}
