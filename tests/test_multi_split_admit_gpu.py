"""The packed split kernel's launch-long admission to its steady loop
(k_step_split_multi, PACK; skrange::admit_* in csrc/sk_range.hpp): a wave
enters the loop only if no state of it can stop fitting the packed form in
the ticks that remain, and the steady tick then carries no fit test and no
exchange-format stores.  One step_multi launch of 12 ticks must equal 12
single steps bit for bit: state planes, every tick's done / winner row, the
RNG step counter and the episode counters (the pattern and helpers of
tests/test_multi_split_collide_gpu.py, the fixtures and the forcing of
tests/multi_split_cases.py: SK_MULTI_SPLIT=1, SK_MULTI_PACK=1,
both trig forms, both state ports, both workgroup sizes; 1, 31, 32, 33 and 65
games).  Tick 0 and tick 11 run the generic tick, ticks 1..10 the steady loop
where the wave is admitted.

  * the age boundary: a game per wave whose post-tick-0 clock is (qcd, qage)
    = (5, 250) is admitted and reaches age 255 inside the loop; (5, 251) is
    not, and reaches 256 at its fifth tick, in the generic tick;
  * the ticks boundary: entry ticks + 12 = 65535 (admitted) and 65536 (not),
    under a tick limit above both, with and without auto-reset;
  * a game that dies inside the loop without auto-reset, with the victim's
    cooldown at 0 in that very tick: the dead game fires once more;
  * restarts inside the loop, and launches chained on one env so that
    admission is decided anew at every launch start with projectiles in
    flight;
  * the host's gates: boards with W - size = 255 (admitted; a move landing on
    255 inside the loop) and 256 (the generic tick for the launch; the move
    lands on 256, which no packed form holds), cooldown_max 127 and 128.
Every crafted event is played first by oracle/pyoracle.py, which must put it
at the tick claimed.  (The moves, projectile steps and collisions on and one
past each bound at ticks 3..8 are test_multi_split_collide_gpu.py's crafted
games, which are all admitted and now run the loop without its fit test.)
"""
import math

import numpy as np
import pytest
import torch

import oracle.pyoracle as pyoracle
from oracle.pyoracle import PyOracle
from multi_split_cases import _env, block, fast, pol  # noqa: F401
from test_multi_split_collide_gpu import P1, P2, T, _check, ssa  # noqa: F401

pytestmark = pytest.mark.gpu

SIZES = [1, 31, 32, 33, 65]


def _wave_heads(n):
    return sorted({0, 32 % n, 64 % n, n - 1})


def _idle(st, acts, g, qcdage, ticks=0):
    """Game g: both players stand still, far apart, nothing in flight."""
    st["pos"][g] = P1 + P2
    st["rot"][g] = 0.0
    st["qpos"][g] = 0
    st["qrot"][g] = 0.0
    st["qcdage"][g] = qcdage
    st["misc"][g] = (ticks, 1 << 16)
    acts[:, :, g, :] = 0.0


def _play(st, acts, games, n_ticks=T, tick_limit=2000):
    """oracle/pyoracle.py on the chosen games, no restarts: the games after every tick."""
    o = PyOracle(len(games))
    o.load({k: np.asarray(v)[games] for k, v in st.items() if k != "step_counter"})
    hist = []
    for t in range(n_ticks):
        o.step(acts[t][:, games, :], tick_limit=tick_limit)
        hist.append([(G.live, G.winner, list(G.x), list(G.y), list(G.qcd), list(G.qage), G.ticks, list(G.qx), list(G.qy))
                     for G in o.games])
    return hist


def _make(ssa, n, seed, tick_limit, config=None):
    kw = {} if config is None else {"config": config}
    a = ssa.VecSkillshotGame(n, seed=seed, tick_limit=tick_limit, **kw)
    a.reset(random_positions=True)
    b = ssa.VecSkillshotGame(n, seed=seed, tick_limit=tick_limit, **kw)
    acts = a.gen_random_actions(T)
    return a, b, acts, a.state_dict(), acts.cpu().numpy()


def _load(a, b, acts, st, an):
    acts.copy_(torch.from_numpy(an))
    for g in (a, b):
        g.load_state_dict(st)
        g.clear_counters()


# ------------------------------------------------------------------ the age boundary
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("age0", [249, 250], ids=["admitted_5_250", "rejected_5_251"])
def test_age_boundary(ssa, monkeypatch, pol, block, fast, n, age0):
    _env(monkeypatch, pol, block, fast)
    a, b, acts, st, an = _make(ssa, n, 31, 2000)
    heads = _wave_heads(n)
    for g in heads:
        _idle(st, an, g, (6, age0, 6, age0))
    h = _play(st, an, heads)
    for i in range(len(heads)):
        assert h[0][i][4] == [5, 5] and h[0][i][5] == [age0 + 1] * 2  # the clock the admission sees
        assert all(h[t][i][0] for t in range(6))
        assert h[5][i][4] == [0, 0] and h[5][i][5] == [age0 + 6] * 2  # 255: fits; 256: its fifth tick after
        assert h[6][i][5] == [1, 1]  # fired at tick 6
    assert age0 + 6 == (255 if age0 == 249 else 256)
    _load(a, b, acts, st, an)
    _check(a, b, acts, T, T, 0)


# ---------------------------------------------------------------- the ticks boundary
@pytest.mark.parametrize("n", [33, 65])
@pytest.mark.parametrize("auto_reset", [False, True], ids=["no_reset", "auto_reset"])
@pytest.mark.parametrize("end", [65535, 65536])
def test_ticks_boundary(ssa, monkeypatch, pol, block, fast, n, auto_reset, end):
    _env(monkeypatch, pol, block, fast)
    a, b, acts, st, an = _make(ssa, n, 37, 70000)
    heads = _wave_heads(n)
    for g in heads:
        _idle(st, an, g, (100, 0, 100, 0), ticks=end - T)
    h = _play(st, an, heads, tick_limit=70000)
    for i in range(len(heads)):
        assert all(h[t][i][0] for t in range(T)) and h[T - 1][i][6] == end
    _load(a, b, acts, st, an)
    done, _ = _check(a, b, acts, T, T, 0, auto_reset)
    assert not done.cpu().numpy()[:, heads].any()
    assert (a.state_dict()["misc"][heads, 0] == end).all()


# ------------------------------------------------- a game dies in the loop and fires once more
@pytest.mark.parametrize("n", [33, 65])
def test_dead_game_fires_in_the_loop(ssa, monkeypatch, pol, block, fast, n):
    _env(monkeypatch, pol, block, fast)
    a, b, acts, st, an = _make(ssa, n, 41, 2000)
    heads, k = _wave_heads(n), 4
    for g in heads:  # player 2's projectile flies up into player 1 at tick k, where player 1's cooldown reaches 0
        _idle(st, an, g, (k + 1, 0, 100, 0))
        st["qpos"][g, 2:4] = (P1[0] + 1, P1[1] + 4 + 5 * (k + 1))
        st["misc"][g] = (0, (1 << 8) | (1 << 16))
    h = _play(st, an, heads)
    for i in range(len(heads)):
        assert all(h[t][i][0] for t in range(k)) and not h[k][i][0] and h[k][i][1] == 1
        assert h[k][i][4][0] == 0  # ... so the dead game fires at tick k + 1, and its clock stands from there
        assert h[k + 1][i][4][0] == 15 and h[k + 1][i][5][0] == 0 and h[T - 1][i][4][0] == 15
    _load(a, b, acts, st, an)
    done, win = _check(a, b, acts, T, T, 0, auto_reset=False)
    d, w = done.cpu().numpy(), win.cpu().numpy()
    assert not d[:k, heads].any() and d[k:, heads].all() and (w[k:, heads] == 1).all()


# ------------------------------------------------------------- restarts, chained launches
@pytest.mark.parametrize("n", SIZES)
def test_restart_inside_the_loop(ssa, monkeypatch, pol, block, fast, n):
    """Tick limit 7: a game restarts at tick 6 unless it was hit before (then there), inside the loop."""
    _env(monkeypatch, pol, block, fast)
    a, b, acts, st, an = _make(ssa, n, 43, 7)
    _load(a, b, acts, st, an)
    done, _ = _check(a, b, acts, T, T, 0)
    assert done.cpu().numpy()[6].any() and a.counters()["dones"] >= n


def test_chained_launches_decide_admission_anew(ssa, monkeypatch, pol, block, fast):
    """4, 12, 5, 9, 3 and 12 ticks on 65 games, tick limit 40: projectiles fired in one launch are in
    flight when the next one decides its admission; a game per wave carries a clock that the second
    launch rejects while the game lives (age 244 + cooldown 12 at its start) and the later ones admit."""
    _env(monkeypatch, pol, block, fast)
    a, b, acts, st, an = _make(ssa, 65, 47, 40)
    acts = a.gen_random_actions(5)
    for g in _wave_heads(65):
        st["qcdage"][g] = (16, 240, 16, 240)
    for g in (a, b):
        g.load_state_dict(st)
        g.clear_counters()
    s = 2
    for n_ticks in (4, 12, 5, 9, 3, 12):
        _check(a, b, acts, n_ticks, 5, s)
        s = (s + n_ticks) % 5
    fl = a.state_dict()["misc"][:, 1]
    assert ((fl & 0x101) != 0).any()  # projectiles in flight at a launch boundary


# ------------------------------------------------------------------------ the host's gates
@pytest.mark.parametrize("board", [260, 261], ids=["room255", "room256"])
def test_board_room_gate(ssa, monkeypatch, pol, block, fast, board):
    """Sizes 5 / 5 on a 260 board: W - size = 255, admitted; on 261 the generic tick.  A player of
    game g moves right onto 255 (256) at tick 4, a projectile steps onto it at tick 5."""
    _env(monkeypatch, pol, block, fast)
    cfg = ssa._capi.default_config()
    cfg.board_w = cfg.board_h = board
    cfg.projectile_size = 5
    n, room = 65, board - 5
    a, b, acts, st, an = _make(ssa, n, 53, 2000, cfg)
    heads = _wave_heads(n)
    for g in heads:
        _idle(st, an, g, (100, 0, 100, 0))
        st["pos"][g, 0] = room - 3  # player 1 looks left of its motion: rot -pi/2 moves +3 in x
        st["rot"][g, 0] = -math.pi / 2
        an[4, 0, g, 0] = 1.0
        st["qpos"][g, 2:4] = (room - 5 * 6, 30)  # player 2's projectile: +5 in x per tick
        st["qrot"][g, 1] = -math.pi / 2
        st["misc"][g] = (0, (1 << 8) | (1 << 16))
    with monkeypatch.context() as m:  # the oracle on this board
        m.setattr(pyoracle, "BOARD", board)
        m.setattr(pyoracle, "PROJ_SIDE", 5)
        h = _play(st, an, heads)
    for i in range(len(heads)):
        assert h[3][i][2][0] == room - 3 and h[4][i][2][0] == room
        assert h[4][i][7][1] == room - 5 and h[5][i][7][1] == room
    _load(a, b, acts, st, an)
    _check(a, b, acts, T, T, 0)
    assert (a.state_dict()["pos"][heads, 0] == room).all()


@pytest.mark.parametrize("cdmax", [127, 128])
@pytest.mark.parametrize("n", [65])
def test_cooldown_gate(ssa, monkeypatch, pol, block, fast, cdmax, n):
    """cooldown_max 127 is admitted, 128 runs the generic tick; every player fires at tick 0."""
    _env(monkeypatch, pol, block, fast)
    cfg = ssa._capi.default_config()
    cfg.cooldown_max = cdmax
    a, b, acts, st, an = _make(ssa, n, 59, 9, cfg)
    _load(a, b, acts, st, an)
    _check(a, b, acts, T, T, 0)
    assert a.counters()["dones"] >= n
