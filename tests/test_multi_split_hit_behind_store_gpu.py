"""The packed split kernel's steady tick (k_step_split_multi, PACK) stores its
state ahead of the collision test, with `live` and `winner` as loaded, and a
game hit in that tick stores its {pos, cah} word again from the done block
(split_tick_carry's STEADY form).  One step_multi launch of 12 ticks must
equal 12 single steps bit for bit: state planes, every tick's done / winner
row, the RNG step counter and the episode counters.  The path is forced with
SK_MULTI_SPLIT=1 and SK_MULTI_PACK=1, for both trig forms (SK_MULTI_FAST
0 / 1), both state ports and both workgroup sizes, at 1, 31, 32, 33 and 65
games (a masked wave, a full wave, and one of each).

Every game of a batch is crafted; its event arises at a tick of the steady
loop (2..10 of 12: not tick 0 or 1, not the last), which oracle/pyoracle.py
confirms first on the CPU:

  * player 1 hit, player 2 hit, both in one tick (player 1 wins); each with
    auto_reset off (the corrected word; the game stays dead and unchanged for
    the remaining ticks) and on (the restart's store wins), with fixed and
    random restart positions;
  * a hit in the tick where `ticks` reaches the tick limit, and the tick
    limit alone (done without a hit: no correction is stored);
  * a hit by a projectile fired in the same tick, and a hit in the tick where
    the victim's own projectile leaves the board (its `qvalid` clears in the
    word that is stored twice);
  * a hit in the first and in the last game of a wave and in the last game of
    a partial wave (games 0, 31, 32, 63, 64 and n - 1 are hit games);
  * a game dead from the launch's start (it takes the done block every tick);
  * a hit in a wave that takes the exact fallback in that tick (the
    half-integer move delta of tests/test_multi_split_rec16_gpu.py);
  * two chained launches with a hit in the last steady tick of the first: its
    generic last tick must write the corrected state out.
"""
import math

import numpy as np
import pytest
import torch

from oracle.pyoracle import PyOracle
from test_multi_fast_trig_gpu import PSPEED, move_safe
from multi_split_cases import _env, block, fast, pol  # noqa: F401

pytestmark = pytest.mark.gpu

T, LIMIT = 12, 2000
P1, P2 = (60, 120), (170, 120)  # the crafted games' players; nobody moves or turns
STEP = {"up": (0.0, (0, -5)), "down": (math.pi, (0, 5)), "left": (math.pi / 2, (-5, 0))}
# victim, the projectile's direction, where it stands relative to the victim when it hits
HITS = {"p1": ([(0, "up", (1, 4))], 1), "p2": ([(1, "left", (3, 2))], 2),
        "both": ([(0, "up", (2, 5)), (1, "down", (-1, 2))], 1)}
KINDS = ["p1", "p2", "both", "limit_hit", "limit_alone", "fired", "qclear", "dead", "fallback"]
EDGE = ["p1", "p2", "both"]


@pytest.fixture(scope="module")
def ssa():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import skillshot_learning_amd as m
    m.load_library()
    cfg = m._capi.default_config()
    assert (cfg.board_w, cfg.board_h, cfg.player_size, cfg.projectile_size) == (250, 250, 5, 3)
    assert (cfg.player_speed, cfg.projectile_speed, cfg.cooldown_max) == (PSPEED, 5, 15)
    return m


def _layout(n, n_ticks=T, last_steady_only=False):
    """[(game, tick, kind)]: the wave's first and last games and the batch's
    last game are plain hits, the others go through KINDS in turn; the ticks
    through the steady loop's (2 .. n_ticks - 2)."""
    edge = sorted({g for g in (0, 31, 32, 63, 64, n - 1) if g < n})
    out = []
    for g in range(n):
        kind = EDGE[(n + edge.index(g)) % 3] if g in edge else KINDS[g % len(KINDS)]
        k = n_ticks - 2 if last_steady_only else 2 + (g * 5) % (n_ticks - 3)
        out.append((g, k, kind))
    return out


def _craft(st, acts, layout):
    """Edit the state and the actions (float32 [T, 2, N, 2] numpy) in place."""
    for g, k, kind in layout:
        st["pos"][g] = P1 + P2
        st["rot"][g] = 0.0
        st["qpos"][g] = 0
        st["qrot"][g] = 0.0
        st["qcdage"][g] = (100, 0, 100, 0)  # nobody fires
        ticks, live, winner, qv = 0, 1, 0, [0, 0]
        acts[:, :, g, :] = 0.0
        hits = HITS.get(kind, HITS["p1"])[0] if kind not in ("limit_alone", "fired", "dead") else []
        for victim, d, (dx, dy) in hits:  # in flight from the start, k + 1 steps from where it hits
            s, v = 1 - victim, (P1, P2)[victim]
            rot, (sx, sy) = STEP[d]
            st["qpos"][g, 2 * s:2 * s + 2] = (v[0] + dx - sx * (k + 1), v[1] + dy - sy * (k + 1))
            st["qrot"][g, s] = rot
            qv[s] = 1
        if kind in ("limit_hit", "limit_alone"):
            ticks = LIMIT - (k + 1)
        elif kind == "fired":  # player 2 stands below player 1 and fires upwards at tick k
            st["pos"][g, 2:4] = (P1[0], P1[1] + 10)
            st["qcdage"][g, 2] = k
        elif kind == "qclear":  # player 1's own projectile, one cell short of the top edge after k steps
            st["qpos"][g, 0:2] = (10, 5 * (k + 1) - 1)
            qv[0] = 1
        elif kind == "dead":
            live, winner = 0, 2
        elif kind == "fallback":  # the shooter's move delta is a half-integer in the tick of the hit
            acts[k, 1, g, 0] = 0.5 / PSPEED
        st["misc"][g] = (ticks, qv[0] | (qv[1] << 8) | (live << 16) | (winner << 24))


def _verify_on_cpu(st, acts, layout, n_ticks=T):
    """oracle/pyoracle.py plays the crafted games without restarts: each event
    happens at the tick claimed, inside the steady loop, and not before."""
    o = PyOracle(len(layout))
    o.load({k: np.asarray(v) for k, v in st.items() if k != "step_counter"})
    hist = []
    for t in range(n_ticks):
        o.step(acts[t])
        hist.append([(G.live, G.winner, G.ticks, list(G.qvalid), list(G.qage)) for G in o.games])
    for g, k, kind in layout:
        h = [hist[t][g] for t in range(n_ticks)]
        assert 2 <= k <= n_ticks - 2, kind
        if kind == "dead":
            assert all(not x[0] and x[1] == 2 and x[2] == 0 for x in h), kind
            continue
        assert all(x[0] and x[1] == 0 for x in h[:k]), (g, kind)  # nothing before tick k
        if kind == "limit_alone":
            assert all(x[0] and x[1] == 0 for x in h), kind
            assert h[k - 1][2] == LIMIT - 1 and h[k][2] == LIMIT, kind
            continue
        want = HITS[kind][1] if kind in HITS else 1
        assert not h[k][0] and h[k][1] == want, (g, kind)
        assert h[k][2] == (LIMIT if kind == "limit_hit" else k + 1), kind
        if kind == "limit_hit":
            assert h[k - 1][2] == LIMIT - 1, kind
        elif kind == "fired":  # no projectile before the tick of the hit; it is one tick old there
            assert not h[k - 1][3][1] and h[k][3][1] and h[k][4][1] == 1, kind
        elif kind == "qclear":
            assert h[k - 1][3][0] and not h[k][3][0], kind
        elif kind == "fallback":
            assert not move_safe(0.0, acts[k, 1, g, 0]), kind


def _pair(ssa, n, seed, random_positions):
    a = ssa.VecSkillshotGame(n, seed=seed, tick_limit=LIMIT, random_positions=random_positions)
    a.reset(random_positions=True)
    b = ssa.VecSkillshotGame(n, seed=seed, tick_limit=LIMIT, random_positions=random_positions)
    return a, b


def _load(a, b, st, acts, an):
    acts.copy_(torch.from_numpy(an))
    for g in (a, b):
        g.load_state_dict(st)
        g.clear_counters()


def _check(a, b, acts, n_ticks, slab0, auto_reset):
    """One launch of n_ticks ticks on `a` against n_ticks single ticks on `b`."""
    R = acts.shape[0]
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
    return done.cpu().numpy(), win.cpu().numpy(), sa


@pytest.mark.parametrize("restart", ["no_reset", "reset_fixed", "reset_random"])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 65])
def test_hits_inside_the_steady_loop(ssa, monkeypatch, pol, block, fast, n, restart):
    _env(monkeypatch, pol, block, fast)
    auto_reset = restart != "no_reset"
    a, b = _pair(ssa, n, 23, restart == "reset_random")
    acts = a.gen_random_actions(T)
    st, an, layout = a.state_dict(), acts.cpu().numpy(), _layout(n)
    _craft(st, an, layout)
    _verify_on_cpu(st, an, layout)
    _load(a, b, st, acts, an)
    d, w, end = _check(a, b, acts, T, 0, auto_reset)
    fl = end["misc"][:, 1].astype(np.int64) & 0xFFFFFFFF
    for g, k, kind in layout:  # the rows say what the oracle said
        if kind == "dead":
            assert d[0, g] == 1 and w[0, g] == 2, kind
            if not auto_reset:
                assert d[:, g].all() and (w[:, g] == 2).all() and end["misc"][g, 0] == 0, kind
            continue
        assert not d[:k, g].any() and not w[:k, g].any() and d[k, g] == 1, (g, kind)
        if kind == "limit_alone":
            assert w[k, g] == 0, kind
            if not auto_reset:  # live past the limit: done on every tick, never hit
                assert d[k:, g].all() and not w[:, g].any() and end["misc"][g, 0] == LIMIT + T - 1 - k, kind
                assert (fl[g] >> 16) & 0xFF == 1, kind
            continue
        want = HITS[kind][1] if kind in HITS else 1
        assert w[k, g] == want, (g, kind)
        if not auto_reset:  # dead and unchanged from tick k on: the corrected word stayed
            assert d[k:, g].all() and (w[k:, g] == want).all(), (g, kind)
            assert (fl[g] >> 16) & 0xFF == 0 and (fl[g] >> 24) & 0xFF == want, (g, kind)
            assert end["misc"][g, 0] == (LIMIT if kind == "limit_hit" else k + 1), (g, kind)
    if auto_reset:
        assert a.counters()["dones"] >= n


def test_hit_in_the_last_steady_tick_of_a_chained_launch(ssa, monkeypatch, pol, block, fast):
    """Two launches of 8 ticks on 65 games without restarts: every hit of the
    first arises at tick 6, its last steady tick, so the generic tick behind
    it reloads the corrected word and writes the exchange format from it; the
    second launch starts from that."""
    _env(monkeypatch, pol, block, fast)
    n, nt = 65, 8
    a, b = _pair(ssa, n, 31, False)
    acts = a.gen_random_actions(nt)
    st, an, layout = a.state_dict(), acts.cpu().numpy(), _layout(n, nt, True)
    _craft(st, an, layout)
    _verify_on_cpu(st, an, layout, nt)
    _load(a, b, st, acts, an)
    d, w, end = _check(a, b, acts, nt, 0, False)
    fl = end["misc"][:, 1].astype(np.int64) & 0xFFFFFFFF
    hit = [g for g, k, kind in layout if kind not in ("dead", "limit_alone")]
    assert len(hit) > 40 and all(d[nt - 2, g] == 1 and w[nt - 2, g] in (1, 2) for g in hit)
    assert all((fl[g] >> 16) & 0xFF == 0 and (fl[g] >> 24) & 0xFF == w[nt - 2, g] for g in hit)
    _check(a, b, acts, nt, 0, False)
