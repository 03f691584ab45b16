"""The packed split kernel's player record (rotation, pack_pos, pack_cah and
the projectile rotation, k_step_split_multi, PACK) and the state-independent
part of its fast steady tick evaluated under the loads (SplitPre): one
step_multi launch must equal one step per tick bit for bit: state
planes, every tick's done / winner row, the RNG step counter and the episode
counters.  The path is forced with SK_MULTI_SPLIT=1 and SK_MULTI_PACK=1, for
both trig forms (SK_MULTI_FAST 0 / 1), both state ports and both workgroup
sizes.

  * every bit of the record: a state at the packed form's limits, each of the
    record's four words different, so a wrong word order or a wrong plane
    offset shows as a plane mismatch;
  * ragged batches with restarts and firing: the record's early store, its
    re-store on restart, the planes' offsets (multiples of 16 n) for odd n;
  * the fast tick's fallbacks arising inside the steady loop (ticks 3-8 of
    12), each checked on the CPU first;
  * launches of 1, 2, 3, 4, 5 and 9 ticks chained on one env: nothing stale
    is read from the previous launch's pack buffer.
"""
import numpy as np
import pytest
import torch

from oracle.pyoracle import Game, PyOracle
from test_multi_fast_trig_gpu import (FAST_RANGE, LOOK, PSPEED, QSPEED, _tie_rotations, clampf, fired_safe,
                                      move_safe, sincos_fast)
from multi_split_cases import _env, block, fast, pol  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ssa():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import skillshot_learning_amd as m
    m.load_library()
    cfg = m._capi.default_config()
    assert (cfg.player_speed, cfg.projectile_speed, cfg.look_speed) == (PSPEED, QSPEED, LOOK)
    return m


def _pair(ssa, n, seed, tick_limit, edit=None):
    """Two equal envs from a random start, with `edit(state)` applied."""
    a = ssa.VecSkillshotGame(n, seed=seed, tick_limit=tick_limit)
    a.reset(random_positions=True)
    b = ssa.VecSkillshotGame(n, seed=seed, tick_limit=tick_limit)
    st = a.state_dict()
    if edit is not None:
        edit(st)
    for g in (a, b):
        g.load_state_dict(st)
    return a, b


def _same_state(x, y):
    """Bitwise: a NaN rotation must match too."""
    sx, sy = x.state_dict(), y.state_dict()
    for k in sx:
        ax, ay = np.ascontiguousarray(sx[k]), np.ascontiguousarray(sy[k])
        assert ax.shape == ay.shape and ax.tobytes() == ay.tobytes(), k


def _stepwise(b, acts, T, R, slab0=0):
    wd, ww = [], []
    for t in range(T):
        o = b.step(acts[(slab0 + t) % R], obs=False, auto_reset=True)
        wd.append(o["done"].clone())
        ww.append(o["winner"].clone())
    return torch.stack(wd), torch.stack(ww)


def _check(a, b, acts, T, R, slab0=0):
    """One launch of T ticks on `a` against T single ticks on `b`."""
    done, win = a.step_multi(acts, n_ticks=T, slab0=slab0, record=True)
    wd, ww = _stepwise(b, acts, T, R, slab0)
    torch.cuda.synchronize()
    assert torch.equal(done, wd), T
    assert torch.equal(win, ww), T
    _same_state(a, b)
    assert a.step_counter == b.step_counter
    assert a.counters() == b.counters()


# ------------------------------------------------------ every bit of the record
N_LIMITS = 33  # 66 lanes: one full wave and two lanes of a second


def _limits_state(st):
    """Fields at the packed form's limits, live games with a winner recorded,
    both projectiles in flight; the players and the projectiles far apart.
    Game 32 (the second wave) reaches age 256 four ticks later than the
    others, so both waves leave the packed form inside the steady loop, at
    different ticks."""
    n = N_LIMITS
    g = np.arange(n)
    late = g == n - 1
    st["pos"][:] = np.stack([10 + g, 20 + 2 * g, 249 - (g % 3), 249 - g], 1)
    st["rot"][:] = np.stack([0.3 + 0.01 * g, -2.1 - 0.02 * g], 1)
    st["qpos"][:] = np.stack([249 - g, 3 + (g % 5), 1 + (g % 4), 246 - 2 * (g % 6)], 1)
    st["qrot"][:] = np.stack([-1.3 - 0.03 * g, 1.7 + 0.01 * g], 1)
    # cooldown at both ends of its range (-128 fires on the first tick), age 254 rising
    age = np.where(late, 250, 254 - (g % 2))
    cd0 = np.where(g % 2 == 0, 127, -128)
    st["qcdage"][:] = np.stack([cd0, age, -1 - cd0, age - 1], 1)
    st["misc"][:, 0] = np.where(late, 65529, 65533 - (g % 3))
    st["misc"][:, 1] = 1 | (1 << 8) | (1 << 16) | ((1 + g % 3) << 24)  # both valid, live, winner 1..3


def _record_words(st):
    """The words of every lane's record as packed (rotation low / high word,
    pack_pos, pack_cah): [n, 2, 4] uint32."""
    n = st["pos"].shape[0]
    w = np.zeros((n, 2, 4), np.uint32)
    fl = st["misc"][:, 1].astype(np.int64) & 0xFFFFFFFF
    flags = (fl & 1) | (((fl >> 8) & 1) << 1) | (((fl >> 16) & 1) << 2) | (((fl >> 24) & 3) << 3)
    for p in (0, 1):
        r = np.ascontiguousarray(st["rot"][:, p]).view(np.uint64)
        w[:, p, 0] = (r & 0xFFFFFFFF).astype(np.uint32)
        w[:, p, 1] = (r >> 32).astype(np.uint32)
        px, py = st["pos"][:, 2 * p].astype(np.int64), st["pos"][:, 2 * p + 1].astype(np.int64)
        qx, qy = st["qpos"][:, 2 * p].astype(np.int64), st["qpos"][:, 2 * p + 1].astype(np.int64)
        w[:, p, 2] = (px | (py << 8) | (qx << 16) | (qy << 24)).astype(np.uint32)
        cd, age = st["qcdage"][:, 2 * p].astype(np.int64) & 0xFF, st["qcdage"][:, 2 * p + 1].astype(np.int64)
        hi = flags if p else st["misc"][:, 0].astype(np.int64)
        w[:, p, 3] = (cd | (age << 8) | (hi << 16)).astype(np.uint32)
    return w


def test_every_bit_of_the_record(ssa, monkeypatch, pol, block, fast):
    """9 ticks from the limits: tick 0 packs (age 255, ticks 65,534 still
    fit), the first wave stops fitting at its first or second steady tick
    (age 256), the second at its fifth, and the exchange format takes over."""
    _env(monkeypatch, pol, block, fast)
    T, R = 9, 4
    a, b = _pair(ssa, N_LIMITS, 7, 65540, _limits_state)
    st = a.state_dict()
    assert st["pos"].max() == 249 and st["qcdage"][:, [0, 2]].min() == -128 and st["qcdage"][:, [0, 2]].max() == 127
    w = _record_words(st)
    for lane in w.reshape(-1, 4):
        assert len(set(lane.tolist())) == 4, lane
    acts = a.gen_random_actions(R)
    a.clear_counters()
    b.clear_counters()
    _check(a, b, acts, T, R, 1)
    end = a.state_dict()
    assert end["misc"][:, 0].max() >= 65536 and end["qcdage"][:, [1, 3]].max() >= 256  # past the packed form


# ------------------------------------------- ragged sizes, restarts and firing
@pytest.mark.parametrize("n", [1, 31, 33, 97])
def test_ragged_sizes_with_restarts(ssa, monkeypatch, pol, block, fast, n):
    """Tick limit 5 over 23 ticks from slab 1 of a ring of 4: every game
    restarts four times (its lanes store their record again) and fires every
    sixteenth tick; the pack buffer's planes start at 16 n and 32 n bytes."""
    _env(monkeypatch, pol, block, fast)
    T, R = 23, 4
    a, b = _pair(ssa, n, 3, 5)
    acts = a.gen_random_actions(R)
    a.clear_counters()
    b.clear_counters()
    _check(a, b, acts, T, R, 1)
    assert a.counters()["dones"] > 0


# ------------------------------------------------ fallbacks in the steady loop
N_FALL, T_FALL = 200, 12
NAN, INF = float("nan"), float("inf")
BELOW = float(np.nextafter(FAST_RANGE, 0.0))  # the largest rotation of the fast range


def _fallback_cases():
    """(game, player, tick, kind, value): the tick lies in 3..8, the games
    are spread over the seven waves, two of them in the ragged last one."""
    ties = [r for r, must in _tie_rotations(QSPEED) if must]
    c = [(3, 0, 3, "nan_move", NAN), (40, 1, 4, "nan_look", NAN), (70, 0, 5, "clamp_move", INF),
         (101, 1, 6, "clamp_look", -INF), (133, 0, 7, "clamp_move", 1.5), (166, 1, 8, "clamp_look", -1.5),
         (194, 0, 5, "range", 1.0), (197, 1, 6, "range", -1.0),
         (11, 0, 3, "move_tie", 0.5 / PSPEED), (55, 1, 8, "move_tie", -0.5 / PSPEED),
         (120, 0, 6, "move_tie", 0.5 / PSPEED), (199, 1, 4, "move_tie", 0.5 / PSPEED)]
    for i, (g, p, k) in enumerate([(20, 0, 4), (64, 1, 7), (90, 0, 5), (150, 1, 3), (180, 0, 8), (198, 0, 6)]):
        c.append((g, p, k, "fired_tie", ties[(7 * i) % len(ties)]))
    assert len({g for g, *_ in c}) == len(c)
    return c


FIRE_LOOK = 0.5  # the look action of the tick a "fired_tie" lane fires on


def _fallback_state(st, cases):
    """The crafted games: players far apart and no projectile in flight (no
    hit within 12 ticks), cooldown 100 (no shot) unless the case fires."""
    for g, p, k, kind, v in cases:
        st["pos"][g] = (40, 60, 200, 190)
        st["rot"][g] = (0.0, 0.0)
        st["qpos"][g] = 0
        st["qrot"][g] = 0.0
        st["qcdage"][g] = (100, 0, 100, 0)
        st["misc"][g] = (0, 1 << 16)
        if kind == "range":  # look +-1 every tick: in range up to tick k - 1, outside from tick k
            st["rot"][g, p] = v * (BELOW - 0.25 * (k - 1))
        elif kind == "fired_tie":  # fires at tick k, its rotation then v
            st["rot"][g, p] = v - FIRE_LOOK * LOOK
            st["qcdage"][g, 2 * p] = k
        elif kind == "nan_look":  # fires at tick k with a NaN rotation
            st["rot"][g, p] = 0.7
            st["qcdage"][g, 2 * p] = k


def _fallback_actions(acts, cases):
    """acts: float32 [T, 2, N, 2] numpy, edited in place.  A crafted lane
    looks nowhere (its rotation stays as loaded) except where its case says."""
    for g, p, k, kind, v in cases:
        acts[:, p, g, 1] = 0.0
        if kind in ("nan_move", "clamp_move", "move_tie"):
            acts[k, p, g, 0] = v
        elif kind in ("nan_look", "clamp_look"):
            acts[k, p, g, 1] = v
        elif kind == "range":
            acts[:, p, g, 1] = v
        elif kind == "fired_tie":
            acts[k, p, g, 1] = FIRE_LOOK


def _verify_cases_on_cpu(st, acts, cases):
    """oracle/pyoracle.py plays the crafted games (the protocol's tick in
    Python floats) up to each case's tick; there the lane's rotation and
    cooldown are read from it and the kernel's fp32 decisions (the formulas of
    tests/test_multi_fast_trig_gpu.py) are evaluated on them with the tick's
    action: the game is live and not restarted, and the case takes the branch
    it is meant for at tick k, and, where it is an event, not before."""
    games = sorted({g for g, *_ in cases})
    o = PyOracle(len(games))
    o.load({k: np.asarray(v)[games] for k, v in st.items() if k != "step_counter"})
    by_tick = {}
    for c in cases:
        by_tick.setdefault(c[2], []).append(c)
    retired = set()
    for t in range(T_FALL):
        for g, p, k, kind, v in by_tick.get(t, []):
            G = o.games[games.index(g)]
            assert isinstance(G, Game) and G.live and G.ticks == t, (g, kind)
            rot, am, al = G.rot[p], acts[t, p, g, 0], acts[t, p, g, 1]
            fires = G.qcd[p] <= 0
            if kind == "nan_move":
                assert not move_safe(rot, am)
            elif kind == "nan_look":
                assert fires and not fired_safe(rot, al)
            elif kind == "clamp_move":
                assert clampf(am) != np.float32(am) and abs(clampf(am)) == 1.0 and move_safe(rot, am)
            elif kind == "clamp_look":
                assert clampf(al) != np.float32(al) and abs(clampf(al)) == 1.0 and not fires
            elif kind == "range":
                assert abs(rot) > 1647099 and not sincos_fast(rot)[2]
                assert sincos_fast(rot - v * 0.25)[2]  # the tick before was inside
            elif kind == "move_tie":
                assert rot == 0.0 and not move_safe(rot, am)
                d = np.float32(np.float32(PSPEED) * clampf(am))
                assert abs(abs(float(d)) - 0.5) <= 1e-6 * PSPEED
            elif kind == "fired_tie":
                assert fires and G.qcd[p] == 0 and not fired_safe(rot, al)
            if not (np.isfinite(am) and np.isfinite(al)):
                retired.add(g)  # Python's round() takes no NaN: the game's later ticks are not needed
        for i, g in enumerate(games):
            if g in retired:
                continue
            G = o.games[i]
            for p in (0, 1):
                G.move_direction(p, float(acts[t, p, g, 0]))
                G.move_look(p, float(acts[t, p, g, 1]))
                G.shoot(p)
            G.game_tick()
            assert G.live, (g, t)  # no restart: the rotations stay what the cases need


def test_fallbacks_inside_the_steady_loop(ssa, monkeypatch, pol, block, fast):
    """Non-finite and out-of-range actions, a rotation leaving the fast range,
    a move delta at a half-integer and a fired step next to one, each arising
    at a tick of the steady loop (3..8 of 12) in a wave that ran the fast
    path until then: the state-independent part evaluated under the loads must
    send the wave to the exact evaluation exactly as the generic tick does."""
    cases = _fallback_cases()
    _env(monkeypatch, pol, block, fast)
    a, b = _pair(ssa, N_FALL, 19, 2000, lambda st: _fallback_state(st, cases))
    acts = a.gen_random_actions(T_FALL)
    an = acts.cpu().numpy()
    _fallback_actions(an, cases)
    _verify_cases_on_cpu(a.state_dict(), an, cases)
    acts.copy_(torch.from_numpy(an))
    a.clear_counters()
    b.clear_counters()
    _check(a, b, acts, T_FALL, T_FALL)


# --------------------------------------------------- chained launches, one env
def test_chained_launches_on_one_env(ssa, monkeypatch, pol, block, fast):
    """1, 2, 3, 4, 5 and 9 ticks follow each other on 97 games with restarts
    (tick limit 6): a 1-tick launch never packs, a 2-tick one has no steady
    tick, and each starts from the exchange format, whatever the previous
    launch left in the pack buffer."""
    _env(monkeypatch, pol, block, fast)
    n, R = 97, 5
    a, b = _pair(ssa, n, 11, 6)
    acts = a.gen_random_actions(R)
    a.clear_counters()
    b.clear_counters()
    s = 3
    for T in (1, 2, 3, 4, 5, 9, 1, 9):
        _check(a, b, acts, T, R, s)
        s = (s + T) % R
    assert a.counters()["dones"] > 0
