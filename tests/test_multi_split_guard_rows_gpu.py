"""The packed split kernel's steady tick (k_step_split_multi, PACK) decides
under its loads which lanes may need the exact evaluation (`maybe`: an unsafe
move delta, an unsafe fired step, a flagged projectile in flight) and takes the
exactness guard `un` only in a wave-tick where some lane may; it addresses the
action ring and the done / winner rows with wave-uniform 32-bit offsets that
wrap inside the loop, and a NULL row's stores are dropped
(csrc/sk_multi.hpp).  One sk_env_step_multi launch of 12 ticks must equal 12
single steps bit for bit: state planes, done / winner rows, the RNG step
counter and the episode counters.  The path is forced with SK_MULTI_SPLIT=1
and SK_MULTI_PACK=1, for both trig forms (SK_MULTI_FAST 0 / 1) and both state
ports, at 1, 31, 32, 33 and 65 games (a masked wave, a full wave, one of
each); ticks 1..10 of 12 run the steady loop.

The guard.  Every game of a batch is crafted and played first by
oracle/pyoracle.py, which must put each event at the tick claimed, inside the
steady loop; the rotations next to a half-integer step are found the way
tests/test_multi_fast_trig_gpu.py finds its own, and a host build of
csrc/sk_trig.hpp (the kernels' own fast_move_delta / fast_step_delta) says
for each crafted (rotation, action) on which side of its bound it lands:

  * near_nofire   a player whose fired step would be within its bound of a
                  half-integer and who never fires: `maybe` on every tick, `un`
                  on none;
  * near_fire     the same player firing at tick k: both, and the projectile
                  stays flagged for its flight;
  * qex_invalid   a flagged projectile in flight that leaves the board at
                  tick k: flagged and `un` up to k, `maybe` alone after it;
  * unsafe_move   a move delta of a half-integer at tick k;
  * restart_flag  a game that reaches the tick limit at tick k - 1 and
                  restarts, with an unsafe move at tick k;
  * idle          nothing: the lanes around the others;
  * a batch where only the last in-range lane is ever flagged (the last lane
    of a partial wave at 1, 31, 33 and 65 games).

The rows and the ring.  Random play with restarts on a ring of 5 slabs (it
wraps twice inside the loop), out_stride 0 and n (sk_env_step_multi_obs runs
the obs kernel, so the step-only launch's row offset is exercised through its
two strides), done and winner each NULL or not, and two chained launches that
start from different slabs.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle.pyoracle import PyOracle
from multi_split_cases import _env, block, fast, pol  # noqa: F401
from test_multi_fast_trig_gpu import LOOK, PSPEED, QSPEED, _tie_rotations

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, LIMIT = 12, 2000
SIZES = [1, 31, 32, 33, 65]
P1, P2 = (60, 120), (170, 120)  # the crafted games' players; nobody turns
KINDS = ["near_nofire", "near_fire", "qex_invalid", "unsafe_move", "restart_flag", "idle"]
HALF_MOVE = 0.5 / PSPEED  # at rotation 0 the move's y delta is 0.5

HOST_SRC = r"""
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "sk_trig.hpp"
// argv: triples (rotation, move action, look action), speeds and look speed first.
// Per triple: the move's `safe`, the fired step's, and the in-flight step's of a
// projectile with that rotation (split_fast_pre and the key-miss block).
static float clampf(float a) { a = a >= 1.0f ? 1.0f : a; return a <= -1.0f ? -1.0f : a; }
int main(int argc, char** argv) {
  const float ps = (float)atof(argv[1]), qs = (float)atof(argv[2]);
  const double look = atof(argv[3]);
  for (int i = 4; i + 2 < argc; i += 3) {
    const double rot = strtod(argv[i], 0);
    const float am = (float)strtod(argv[i + 1], 0), al = (float)strtod(argv[i + 2], 0);
    bool ok;
    const sktrig::SinCosF m = sktrig::sincos_fast(rot, &ok);
    const sktrig::FastDelta dm = sktrig::fast_move_delta(m, ok, ps, clampf(am));
    const sktrig::SinCosF u = sktrig::sincos_add(m, clampf(al) * (float)look);
    printf("%d %d %d\n", (int)dm.safe, (int)sktrig::fast_step_delta(u, ok, qs).safe,
           (int)sktrig::fast_step_delta(m, ok, qs).safe);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def ssa():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import skillshot_learning_amd as m
    m.load_library()
    cfg = m._capi.default_config()
    assert (cfg.board_w, cfg.board_h, cfg.player_size, cfg.projectile_size) == (250, 250, 5, 3)
    assert (cfg.player_speed, cfg.projectile_speed, cfg.look_speed, cfg.cooldown_max) == (PSPEED, QSPEED, LOOK, 15)
    return m


@pytest.fixture(scope="module")
def decisions(tmp_path_factory):
    """(rotation, move action, look action) -> (move safe, fired step safe,
    in-flight step safe), from the host build of csrc/sk_trig.hpp."""
    d = tmp_path_factory.mktemp("guard_rows")
    src, exe = str(d / "decide.cpp"), str(d / "decide")
    with open(src, "w") as f:
        f.write(HOST_SRC)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I",
                    os.path.join(ROOT, "skillshot_learning_amd", "csrc"), "-o", exe, src, "-lm"], check=True)

    def ask(triples):
        args = [repr(float(x)) for t in triples for x in t]
        out = subprocess.run([exe, str(PSPEED), str(QSPEED), repr(LOOK)] + args, capture_output=True, text=True,
                             check=True).stdout.split()
        assert len(out) == 3 * len(triples)
        return [tuple(bool(int(v)) for v in out[3 * i:3 * i + 3]) for i in range(len(triples))]

    return ask


@pytest.fixture(scope="module")
def near(decisions):
    """A rotation whose sine times the projectile speed is within the fired
    step's bound of a half-integer (must_fail of _tie_rotations), pointing
    upwards: with no move and no look the move is safe, the fired step and
    the step in flight are not; 1e-3 away all three are safe."""
    cands = [r for r, must in _tie_rotations(QSPEED) if must and 0.0 < r < 0.2]
    assert cands
    r = cands[0]
    assert abs(math.sin(r) * QSPEED - 0.5) < 1e-6
    assert decisions([(r, 0.0, 0.0), (r + 1e-3, 0.0, 0.0)]) == [(True, False, False), (True, True, True)]
    # the crafted moves: a half-integer delta at rotation 0, nothing at action 0
    assert decisions([(0.0, HALF_MOVE, 0.0), (0.0, 0.0, 0.0)]) == [(False, True, True), (True, True, True)]
    return r


def _layout(n):
    """[(game, tick, kind)]: KINDS in turn, the ticks through the steady loop's."""
    out = []
    for g in range(n):
        kind = KINDS[g % len(KINDS)]
        k = 2 + (g * 5) % (T - 3)
        out.append((g, max(k, 3) if kind == "restart_flag" else k, kind))
    return out


def _idle(st, acts, g):
    st["pos"][g] = P1 + P2
    st["rot"][g] = 0.0
    st["qpos"][g] = 0
    st["qrot"][g] = 0.0
    st["qcdage"][g] = (100, 0, 100, 0)  # nobody fires
    st["misc"][g] = (0, 1 << 16)
    acts[:, :, g, :] = 0.0


def _craft_one(st, acts, g, k, kind, near, p=0):
    """Player p of game g (its partner stays idle)."""
    _idle(st, acts, g)
    if kind in ("near_nofire", "near_fire"):
        st["rot"][g, p] = near
        if kind == "near_fire":
            st["qcdage"][g, 2 * p] = k  # fires at tick k, upwards and a little to the left
    elif kind == "qex_invalid":  # in flight from the start, one cell short of the top edge after k steps
        st["qrot"][g, p] = near
        st["qpos"][g, 2 * p:2 * p + 2] = (30 + 100 * p, 5 * (k + 1) - 1)
        st["misc"][g, 1] = (1 << 16) | (1 << (8 * p))
    elif kind == "unsafe_move":
        acts[k, p, g, 0] = HALF_MOVE
    elif kind == "restart_flag":
        st["misc"][g, 0] = LIMIT - k  # the limit at tick k - 1
        acts[k, p, g, 0] = HALF_MOVE


def _verify_on_cpu(st, acts, layout, p_of=lambda g: 0):
    """oracle/pyoracle.py plays the crafted games without restarts."""
    o = PyOracle(len(st["pos"]))
    o.load({k: np.asarray(v) for k, v in st.items() if k != "step_counter"})
    hist = []
    for t in range(T):
        o.step(acts[t], tick_limit=LIMIT)
        hist.append([(G.live, G.ticks, list(G.qvalid), list(G.qage), list(G.y)) for G in o.games])
    for g, k, kind in layout:
        h, p = [hist[t][g] for t in range(T)], p_of(g)
        assert 2 <= k <= T - 2, kind
        assert all(x[0] for x in h), (g, kind)  # nobody is hit
        if kind == "near_nofire":
            assert not any(x[2][p] for x in h), kind
        elif kind == "near_fire":  # no projectile before tick k; one tick old there, and in flight to the end
            assert not h[k - 1][2][p] and h[k][3][p] == 1 and all(x[2][p] for x in h[k:]), (g, kind)
        elif kind == "qex_invalid":
            assert all(x[2][p] for x in h[:k]) and not any(x[2][p] for x in h[k:]), (g, kind)
        elif kind == "unsafe_move":  # 120 less the float32 action's 0.5000000149: the fp64 expression decides
            assert h[k - 1][4][p] == 120 and h[k][4][p] == 119 and h[-1][4][p] == 119, (g, kind)
        elif kind == "restart_flag":
            assert k >= 3 and h[k - 2][1] == LIMIT - 1 and h[k - 1][1] == LIMIT, (g, kind)


def _pair(ssa, n, seed, tick_limit=LIMIT, random_positions=False):
    a = ssa.VecSkillshotGame(n, seed=seed, tick_limit=tick_limit, random_positions=random_positions)
    a.reset(random_positions=True)
    b = ssa.VecSkillshotGame(n, seed=seed, tick_limit=tick_limit, random_positions=random_positions)
    return a, b


def _load(a, b, st):
    for g in (a, b):
        g.load_state_dict(st)
        g.clear_counters()


def _same(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        x, y = np.ascontiguousarray(sa[k]), np.ascontiguousarray(sb[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k
    assert a.step_counter == b.step_counter
    assert a.counters() == b.counters()


def _stepwise(b, acts, n_ticks, slab0=0):
    wd, ww = [], []
    for t in range(n_ticks):
        o = b.step(acts[(slab0 + t) % acts.shape[0]], obs=False, auto_reset=True)
        wd.append(o["done"].clone())
        ww.append(o["winner"].clone())
    return torch.stack(wd), torch.stack(ww)


def _check(a, b, acts, n_ticks=T, slab0=0):
    done, win = a.step_multi(acts, n_ticks=n_ticks, slab0=slab0, record=True)
    wd, ww = _stepwise(b, acts, n_ticks, slab0)
    torch.cuda.synchronize()
    assert torch.equal(done, wd) and torch.equal(win, ww)
    _same(a, b)
    return done.cpu().numpy()


# ------------------------------------------------------------------ the guard
@pytest.mark.parametrize("restart", ["reset_fixed", "reset_random"])
@pytest.mark.parametrize("n", SIZES)
def test_guard_cases_inside_the_steady_loop(ssa, near, monkeypatch, pol, block, fast, n, restart):
    _env(monkeypatch, pol, block, fast)
    a, b = _pair(ssa, n, 29, random_positions=restart == "reset_random")
    acts = a.gen_random_actions(T)
    st, an, layout = a.state_dict(), acts.cpu().numpy(), _layout(n)
    for g, k, kind in layout:
        _craft_one(st, an, g, k, kind, near, p=g % 2)
    _verify_on_cpu(st, an, layout, p_of=lambda g: g % 2)
    acts.copy_(torch.from_numpy(an))
    _load(a, b, st)
    d = _check(a, b, acts)
    for g, k, kind in layout:  # done only where the limit was reached
        want = np.zeros(T, np.uint8)
        if kind == "restart_flag":
            want[k - 1] = 1
        assert np.array_equal(d[:, g], want), (g, kind)
    assert a.counters()["dones"] == sum(kind == "restart_flag" for _, _, kind in layout)


@pytest.mark.parametrize("kind", ["near_fire", "qex_invalid", "unsafe_move"])
@pytest.mark.parametrize("n", SIZES)
def test_only_the_last_lane_is_flagged(ssa, near, monkeypatch, pol, fast, n, kind):
    """Every game idle but the last one, whose player 2 (the last in-range
    lane of the batch's last wave) carries the case at tick 6."""
    _env(monkeypatch, pol, "64", fast)
    a, b = _pair(ssa, n, 37)
    acts = a.gen_random_actions(T)
    st, an = a.state_dict(), acts.cpu().numpy()
    for g in range(n):
        _idle(st, an, g)
    _craft_one(st, an, n - 1, 6, kind, near, p=1)
    _verify_on_cpu(st, an, [(n - 1, 6, kind)], p_of=lambda g: 1)
    acts.copy_(torch.from_numpy(an))
    _load(a, b, st)
    assert not _check(a, b, acts).any()


# ------------------------------------------------------- the ring and the rows
def _raw(g, acts, n_ticks, slab0, done, winner, stride):
    g.step_multi_raw(ctypes.c_void_p(acts.data_ptr()), acts.shape[0], slab0, n_ticks,
                     ctypes.c_void_p(done.data_ptr()) if done is not None else None,
                     ctypes.c_void_p(winner.data_ptr()) if winner is not None else None, stride)


@pytest.mark.parametrize("n", SIZES)
def test_ring_wraps_and_null_rows(ssa, monkeypatch, pol, fast, n):
    """Tick limit 5 over 12 ticks from slab 1 of a ring of 5: the ring wraps
    twice inside the loop and every game restarts twice.  Each of the eight
    launches (done / winner NULL or not, out_stride 0 or n) goes on from the
    state the one before left, against single steps on the twin env; a row
    that is not NULL holds every tick's value (stride n) or the last tick's
    (stride 0), and nothing is written past it."""
    _env(monkeypatch, pol, "64", fast)
    R, slab = 5, 1
    a, b = _pair(ssa, n, 41, tick_limit=5, random_positions=True)
    _load(a, b, a.state_dict())
    acts = a.gen_random_actions(R)
    for stride in (0, n):
        rows = T if stride else 1
        for has_done, has_winner in ((True, False), (False, True), (False, False), (True, True)):
            done = torch.full((rows + 1, n), 0xAB, dtype=torch.uint8, device="cuda") if has_done else None
            win = torch.full((rows + 1, n), 0xAB, dtype=torch.uint8, device="cuda") if has_winner else None
            _raw(a, acts, T, slab, done, win, stride)
            wd, ww = _stepwise(b, acts, T, slab)
            torch.cuda.synchronize()
            for got, want in ((done, wd), (win, ww)):
                if got is not None:
                    assert torch.equal(got[:rows], want if stride else want[-1:]), (stride, has_done, has_winner)
                    assert bool((got[rows] == 0xAB).all())
            _same(a, b)
            slab = (slab + T) % R
    assert a.counters()["dones"] >= 2 * 8 * n


@pytest.mark.parametrize("n", SIZES)
def test_chained_launches_from_different_slabs(ssa, monkeypatch, pol, fast, n):
    """12 ticks from slab 3 of a ring of 5, then 8 ticks from slab 0 where the
    first launch stopped, projectiles in flight across the boundary."""
    _env(monkeypatch, pol, "64", fast)
    a, b = _pair(ssa, n, 43, tick_limit=7, random_positions=True)
    _load(a, b, a.state_dict())
    acts = a.gen_random_actions(5)
    _check(a, b, acts, 12, 3)
    _check(a, b, acts, 8, 0)
    assert a.counters()["dones"] >= 2 * n
