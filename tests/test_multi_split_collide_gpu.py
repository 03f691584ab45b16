"""The packed split kernel's steady tick (k_step_split_multi, PACK) with one
collision test per lane of a pair, one-compare range tests (csrc/sk_range.hpp)
and a full-wave form without the lane mask: one step_multi launch of 12 ticks
must equal 12 single steps bit for bit: state planes, every tick's done /
winner row, the RNG step counter and the episode counters.  The path is
forced with SK_MULTI_SPLIT=1 and SK_MULTI_PACK=1, for both trig forms
(SK_MULTI_FAST 0 / 1), both state ports and both workgroup sizes.

  * 1, 31, 32, 33 and 65 games: a partial wave only, a full wave only, a full
    wave plus two lanes, two full waves plus two lanes, with restarts and
    firing, and a game per wave whose projectile age leaves the packed form
    at the third tick (the wave leaves the steady loop and comes back after
    the restart): the full-wave and the masked steady tick both run, are left
    and re-entered;
  * collisions crafted to arise at ticks 3..8, inside the steady loop:
    player 1 only, player 2 only, both in one tick (player 1 wins), a
    projectile touching each edge of the player's box, one cell outside each
    edge, an overlapping projectile that is invalid, a hit in a game that is
    not live; each played first by oracle/pyoracle.py, which must put the
    event at the tick claimed;
  * a move and a projectile step landing exactly on, and one past, each of
    the four board bounds at ticks 3..8, confirmed the same way;
  * launches chained on one env with projectiles in flight: every launch's
    first tick misses the carry's keys and refreshes them, the steady ticks
    behind it check them on every tick.  (Between two ticks of one launch the
    keys cannot miss: the tick stores the very rotations it keys, also after
    a restart, so the steady loop's own cold block is not reachable through
    the API; the launch start is where the existing tests force the miss.)
"""
import math

import numpy as np
import pytest
import torch

from oracle.pyoracle import PyOracle
from multi_split_cases import _env, block, fast, pol  # noqa: F401

pytestmark = pytest.mark.gpu

T, N_CRAFT = 12, 97
P1, P2 = (60, 120), (170, 120)  # the crafted games' players, idle unless the case moves one
STEP = {"up": (0.0, (0, -5)), "down": (math.pi, (0, 5)), "left": (math.pi / 2, (-5, 0)), "right": (-math.pi / 2, (5, 0))}


@pytest.fixture(scope="module")
def ssa():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import skillshot_learning_amd as m
    m.load_library()
    cfg = m._capi.default_config()
    assert (cfg.board_w, cfg.board_h, cfg.player_size, cfg.projectile_size) == (250, 250, 5, 3)
    assert (cfg.player_speed, cfg.projectile_speed, cfg.cooldown_max) == (3, 5, 15)
    return m


def _pair(ssa, n, seed, tick_limit, edit=None):
    a = ssa.VecSkillshotGame(n, seed=seed, tick_limit=tick_limit)
    a.reset(random_positions=True)
    b = ssa.VecSkillshotGame(n, seed=seed, tick_limit=tick_limit)
    st = a.state_dict()
    if edit is not None:
        edit(st)
    for g in (a, b):
        g.load_state_dict(st)
        g.clear_counters()
    return a, b


def _check(a, b, acts, n_ticks, R, slab0=0, auto_reset=True):
    """One launch of n_ticks ticks on `a` against n_ticks single ticks on `b`."""
    done, win = a.step_multi(acts, n_ticks=n_ticks, slab0=slab0, record=True, auto_reset=auto_reset)
    wd, ww = [], []
    for t in range(n_ticks):
        o = b.step(acts[(slab0 + t) % R], obs=False, auto_reset=auto_reset)
        wd.append(o["done"].clone())
        ww.append(o["winner"].clone())
    torch.cuda.synchronize()
    assert torch.equal(done, torch.stack(wd)), n_ticks
    assert torch.equal(win, torch.stack(ww)), n_ticks
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        x, y = np.ascontiguousarray(sa[k]), np.ascontiguousarray(sb[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k
    assert a.step_counter == b.step_counter
    assert a.counters() == b.counters()
    return done, win


# ----------------------------------------------- full and partial waves, left and re-entered
@pytest.mark.parametrize("n", [1, 31, 32, 33, 65])
def test_full_and_partial_waves(ssa, monkeypatch, pol, block, fast, n):
    """Tick limit 5 over 12 ticks from slab 1 of a ring of 4: every game
    restarts twice and fires after each restart.  The first game of each wave
    and the batch's last game carry a projectile of age 253 that cannot fire:
    age 256 at the third tick does not fit the packed form, so their waves
    leave the steady loop there and return after the restart at the fifth."""
    _env(monkeypatch, pol, block, fast)

    def edit(st):
        for g in sorted({0, 32 % n, 64 % n, n - 1}):
            st["qcdage"][g] = (100, 253, 100, 7)
            st["misc"][g, 1] = 1 | (1 << 8) | (1 << 16)

    a, b = _pair(ssa, n, 3, 5, edit)
    acts = a.gen_random_actions(4)
    _check(a, b, acts, T, 4, 1)
    assert a.counters()["dones"] >= 2 * n


# ------------------------------------------------------------ crafted collisions and bounds
def _cases():
    """(kind, name, ...) per crafted game; its game index and tick follow from its place in the list."""
    c = [("hit", "p1_only", [(0, "up", (1, 4))], 1),
         ("hit", "p2_only", [(1, "left", (3, 2))], 2),
         ("hit", "both", [(0, "up", (2, 5)), (1, "down", (-1, 2))], 1),
         ("hit", "edge_left", [(0, "up", (-3, 4))], 1),
         ("hit", "edge_right", [(1, "down", (5, 4))], 2),
         ("hit", "edge_top", [(0, "right", (0, 0))], 1),
         ("hit", "edge_bottom", [(1, "left", (3, 8))], 2),
         ("pass", "out_left", [(0, "up", (-4, 4))], 0),
         ("pass", "out_right", [(1, "down", (6, 4))], 0),
         ("pass", "out_top", [(0, "right", (0, -1))], 0),
         ("pass", "out_bottom", [(1, "left", (3, 9))], 0),
         ("invalid", "invalid_overlap", [(0, "up", (1, 4))], 0),
         ("dead", "dead_hit", [(0, "up", (1, 4))], 2)]
    for i, (d, lo) in enumerate([("up", True), ("down", False), ("left", True), ("right", False)]):
        for past in (False, True):
            c.append(("move", f"move_{d}_{'past' if past else 'on'}", i % 2, d, lo, past))
            c.append(("proj", f"proj_{d}_{'past' if past else 'on'}", (i + 1) % 2, d, lo, past))
    return [(96 - 3 * i, 3 + i % 6, x) for i, x in enumerate(c)]  # games 96 (the partial wave), 93, ... 12


def _craft(st, acts):
    """Edit the state and the actions (float32 [T, 2, N, 2] numpy) in place."""
    for g, k, x in _cases():
        kind = x[0]
        st["pos"][g] = P1 + P2
        st["rot"][g] = 0.0
        st["qpos"][g] = 0
        st["qrot"][g] = 0.0
        st["qcdage"][g] = (100, 0, 100, 0)  # nobody fires
        live, winner, qv = 1, 0, [0, 0]
        acts[:, :, g, :] = 0.0
        if kind in ("hit", "pass", "invalid", "dead"):
            for victim, d, (dx, dy) in x[2]:
                s, v = 1 - victim, (P1, P2)[victim]
                rot, (sx, sy) = STEP[d]
                back = 0 if kind in ("invalid", "dead") else k + 1  # these overlap from the start
                st["qpos"][g, 2 * s:2 * s + 2] = (v[0] + dx - sx * back, v[1] + dy - sy * back)
                st["qrot"][g, s] = rot
                qv[s] = 0 if kind == "invalid" else 1
            if kind == "dead":
                live, winner = 0, x[3]
        elif kind == "move":
            _, _, p, d, lo, past = x
            axis = 1 if d in ("up", "down") else 0
            st["rot"][g, p] = 0.0 if axis else math.pi / 2
            st["pos"][g, 2 * p + axis] = (3 - past) if lo else (242 + past)
            acts[k, p, g, 0] = 1.0 if lo else -1.0
        else:
            _, _, p, d, lo, past = x
            axis = 1 if d in ("up", "down") else 0
            st["qrot"][g, p] = STEP[d][0]
            st["qpos"][g, 2 * p:2 * p + 2] = (10, 30)
            st["qpos"][g, 2 * p + axis] = (5 * (k + 1) - past) if lo else (247 - 5 * (k + 1) + past)
            qv[p] = 1
        st["misc"][g] = (0, qv[0] | (qv[1] << 8) | (live << 16) | (winner << 24))


def _verify_on_cpu(st, acts):
    """oracle/pyoracle.py plays the crafted games without restarts: each
    event happens at the tick claimed and not before."""
    cases = _cases()
    games = [g for g, _, _ in cases]
    o = PyOracle(len(games))
    o.load({k: np.asarray(v)[games] for k, v in st.items() if k != "step_counter"})
    hist = []
    for t in range(T):
        o.step(acts[t][:, games, :])
        hist.append([(G.live, G.winner, list(G.x), list(G.y), list(G.qx), list(G.qy), list(G.qvalid)) for G in o.games])
    for i, (g, k, x) in enumerate(cases):
        kind, name = x[0], x[1]
        h = [hist[t][i] for t in range(T)]
        assert 3 <= k <= 8
        if kind == "hit":
            assert all(h[t][0] for t in range(k)) and not h[k][0] and h[k][1] == x[3], name
            for victim, d, (dx, dy) in x[2]:  # where the projectile stands when it hits
                s, v = 1 - victim, (P1, P2)[victim]
                assert (h[k][4][s] - v[0], h[k][5][s] - v[1]) == (dx, dy) and h[k][6][s], name
        elif kind in ("pass", "invalid"):
            assert all(h[t][0] and h[t][1] == 0 for t in range(T)), name
            victim, d, (dx, dy) = x[2][0]
            s, v = 1 - victim, (P1, P2)[victim]
            assert (h[k][4][s] - v[0], h[k][5][s] - v[1]) == (dx, dy), name  # beside the box at tick k
            assert h[k][6][s] == (kind == "pass"), name
        elif kind == "dead":
            assert all(not h[t][0] and h[t][1] == x[3] for t in range(T)), name
        elif kind == "move":
            _, _, p, d, lo, past = x
            axis = 1 if d in ("up", "down") else 0
            at = lambda t: (h[t][3] if axis else h[t][2])[p]
            start = (3 - past) if lo else (242 + past)
            assert at(k - 1) == start, name
            assert at(k) == (start if past else (0 if lo else 245)), name
        else:
            _, _, p, d, lo, past = x
            axis = 1 if d in ("up", "down") else 0
            at = lambda t: (h[t][5] if axis else h[t][4])[p]
            assert h[k - 1][6][p], name
            if past:
                assert not h[k][6][p] and at(k) == at(k - 1), name  # the step one past the bound is not taken
            else:
                assert h[k][6][p] and at(k) == (0 if lo else 247) and not h[k + 1][6][p], name


@pytest.mark.parametrize("auto_reset", [False, True], ids=["no_reset", "auto_reset"])
def test_crafted_collisions_and_bounds(ssa, monkeypatch, pol, block, fast, auto_reset):
    _env(monkeypatch, pol, block, fast)
    a, b = _pair(ssa, N_CRAFT, 23, 2000)
    acts = a.gen_random_actions(T)
    st, an = a.state_dict(), acts.cpu().numpy()
    _craft(st, an)
    _verify_on_cpu(st, an)
    acts.copy_(torch.from_numpy(an))
    for g in (a, b):
        g.load_state_dict(st)
        g.clear_counters()
    done, win = _check(a, b, acts, T, T, 0, auto_reset)
    d, w = done.cpu().numpy(), win.cpu().numpy()
    for g, k, x in _cases():  # the rows say what the oracle said
        if x[0] == "hit":
            assert not d[:k, g].any() and d[k, g] == 1 and w[k, g] == x[3], x[1]
        elif x[0] in ("pass", "invalid"):
            assert not d[:, g].any() and not w[:, g].any(), x[1]
        elif x[0] == "dead":
            assert d[0, g] == 1 and w[0, g] == x[3], x[1]
            if not auto_reset:
                assert d[:, g].all() and (w[:, g] == x[3]).all(), x[1]


# ---------------------------------------------------------- key misses at every launch start
def test_chained_launches_with_projectiles_in_flight(ssa, monkeypatch, pol, block, fast):
    """3, 4, 5, 9, 3 and 12 ticks follow each other on 65 games (tick limit
    40: projectiles fired in one launch are in flight at the start of the
    next, whose first tick misses both keys)."""
    _env(monkeypatch, pol, block, fast)
    a, b = _pair(ssa, 65, 29, 40)
    acts = a.gen_random_actions(5)
    s = 2
    for n_ticks in (3, 4, 5, 9, 3, 12):
        _check(a, b, acts, n_ticks, 5, s)
        s = (s + n_ticks) % 5
    fl = a.state_dict()["misc"][:, 1]
    assert ((fl & 0x101) != 0).any()  # projectiles in flight at a launch boundary
