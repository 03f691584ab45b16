"""The step engine at sk_config values other than the reference's own, against
the C oracle (oracle/skillshot_oracle.c, itself pinned to the reference at
these configurations by tests/golden/cfg_*.npz): the configurations, the
oracle's trajectory at each, what that trajectory must contain, and `play`,
which drives one engine path through it.  Shared by tests/test_config_cpu.py
and tests/test_config_gpu.py.

Every run is the learner protocol under the random policy
(gen_random_actions) with tick limit 40 and random auto-reset, from a start
state that puts games where the edges are (START_BLOCK below).
"""
import functools
import math

import numpy as np

import golden_replay as gr
from oracle import oracle

TICK_LIMIT = 40
OBS_TOL = gr.OBS_TOL  # 1e-5 relative to max(1, |ref|)

# name -> the sk_config fields that differ from the reference's.  The same
# table as tests/golden/make_golden.py's CONFIGS (the cfg_*.npz fixtures;
# test_config_cpu.py checks the two agree).
CONFIGS = dict(
    # x / y and W / H swaps: bounds, inv_W / inv_H, the looking reward's / W, the max_dist rule (width alone).
    # W - player_size > 255: the packed kernel's admission refuses it
    cfg_wide=dict(board_w=320, board_h=180, fixed_p2_x=260, fixed_p2_y=140, rand_hi=175),
    # everything differs at once and admission passes: the steady loop away from the default; 0.4 is inexact in fp32
    cfg_packed=dict(board_w=140, board_h=230, player_size=7, projectile_size=4, player_speed=4, projectile_speed=6,
                    cooldown_max=9, look_speed=0.4, fixed_p1_x=20, fixed_p1_y=30, fixed_p2_x=110, fixed_p2_y=190,
                    rand_lo=10, rand_hi=130),
    # just past pi/4, where sktrig::sincos_add's bound ends, and far past it
    cfg_look08=dict(look_speed=0.8),
    cfg_look3=dict(look_speed=3.0),
    # the fp32 error budget scales with the speeds; box_hit with qsize << psize; cooldown 127 is the admission edge
    cfg_fast=dict(player_size=12, projectile_size=1, player_speed=11, projectile_speed=23, cooldown_max=127),
    cfg_cd128=dict(cooldown_max=128),  # one past the admission gate
    # coordinate differences past 46,340, where an int sum of squares wraps
    cfg_huge=dict(board_w=60000, board_h=50000, player_speed=3000, projectile_speed=9000, fixed_p1_x=5000,
                  fixed_p1_y=4000, fixed_p2_x=55000, fixed_p2_y=45000, rand_lo=1000, rand_hi=49000),
)
NAMES = tuple(CONFIGS)
LOOK_CONFIGS = ("cfg_look08", "cfg_look3")
SEEDS = dict.fromkeys(NAMES, 20)  # chosen so that the oracle's run meets `coverage` (test_config_cpu.py)


def cfg_dict(name):
    return dict(gr.CFG_DEFAULT, **CONFIGS[name])


def sk_config(name):
    """the engine's struct for configuration `name`"""
    return gr.sk_config(cfg_dict(name))


# ---- the start state.  Games in blocks of ten: four with both players on
# opposite walls, turned so that a positive move action pushes into the wall
# and a shot leaves the board at once; one per seat in which the other
# player's projectile, in flight, lands on that seat's player at the first
# tick (placed with the oracle's own first tick); four from the random start.
START_BLOCK = 10
_WALL_ROT = (math.pi / 2, -math.pi / 2, 0.0, math.pi)  # left, right, top, bottom: move = pos - (sin, cos) r * speed * a


def _wall_pos(c, w):
    W, H, ps = c["board_w"], c["board_h"], c["player_size"]
    return ((0, H // 2), (W - ps, H // 2), (W // 2, 0), (W // 2, H - ps))[w]


def start_state(name, n, seed):
    """-> the OracleState every run of configuration `name` starts from (step counter included)"""
    c = cfg_dict(name)
    ref = oracle.OracleState(n, seed=seed, config=c)
    ref.reset(random_positions=True)
    rng = np.random.default_rng(seed)
    for g in range(n):
        k = g % START_BLOCK
        if k < 4:
            ref.pos[g] = _wall_pos(c, k) + _wall_pos(c, k ^ 1)
            ref.rot[g] = (_WALL_ROT[k] + rng.uniform(-0.1, 0.1), _WALL_ROT[k ^ 1] + rng.uniform(-0.1, 0.1))
    # where each player stands after the first tick's move (it does not depend on the projectiles)
    look = ref.copy()
    look.step(ref.gen_random_actions(1)[0], tick_limit=TICK_LIMIT, auto_reset=False)
    qs = c["projectile_speed"]
    for g in range(n):
        k = g % START_BLOCK
        if k in (4, 5):
            victim, shooter = k - 4, 5 - k
            tx, ty = (int(v) + 1 for v in look.pos[g, 2 * victim:2 * victim + 2])
            th = math.atan2(c["board_w"] / 2 - tx, c["board_h"] / 2 - ty)  # the flight comes from the centre's side
            ref.qpos[g, 2 * shooter:2 * shooter + 2] = (tx + round(math.sin(th) * qs), ty + round(math.cos(th) * qs))
            ref.qrot[g, shooter] = th
            ref.qcdage[g, 2 * shooter:2 * shooter + 2] = (5, 1)
            ref.misc[g, 1] = int(oracle.pack_flags(np.array([shooter == 0, shooter == 1]), 1, 0))
    return ref


class Trace:
    """The C oracle's run of one configuration: per tick the actions, the state before the tick, after it
    before any restart (`raw`) and after the restart (`state`), done / winner, obs / obs_reset and both rewards."""


@functools.lru_cache(maxsize=None)
def oracle_trace(name, n, T):
    c = cfg_dict(name)
    ref = start_state(name, n, SEEDS[name])
    tr = Trace()
    tr.name, tr.cfg, tr.n, tr.T, tr.seed = name, c, n, T, SEEDS[name]
    tr.start = {k: v.copy() for k, v in ref.arrays().items()}
    tr.step0 = ref.step_counter
    tr.actions = ref.gen_random_actions(T)  # [T, 2, n, 2]: tick t draws at step counter step0 + t, as its restart
    tr.state, tr.raw, tr.pre, tr.done, tr.winner, tr.obs, tr.obs_reset, tr.reward, tr.reward_simple = \
        [], [], [], [], [], [], [], [], []
    for t in range(T):
        tr.pre.append({k: v.copy() for k, v in ref.arrays().items()})
        raw, simple = ref.copy(), ref.copy()
        raw.step(tr.actions[t], tick_limit=TICK_LIMIT, auto_reset=False)
        tr.raw.append(raw.arrays())
        tr.reward_simple.append(simple.step(tr.actions[t], tick_limit=TICK_LIMIT, auto_reset=True,
                                            reward_kind=1)["reward"])
        out = ref.step(tr.actions[t], tick_limit=TICK_LIMIT, auto_reset=True, random_positions=True,
                       want_reset_obs=True)
        tr.state.append({k: v.copy() for k, v in ref.arrays().items()})
        for key, lst in (("done", tr.done), ("winner", tr.winner), ("obs", tr.obs), ("obs_reset", tr.obs_reset),
                         ("reward", tr.reward)):
            lst.append(out[key])
    tr.counters = [int(x) for x in ref.counters]
    tr.step_end = ref.step_counter
    return tr


def compared(t):
    """the ticks (0-based) whose state / obs are compared: the first 40, then every 10th"""
    return t < 40 or (t + 1) % 10 == 0


# ---- what the oracle's run contains (conditions on the test's own input, asserted by test_config_cpu.py)
def coverage(tr):
    c = tr.cfg
    W, H, ps, qsz = c["board_w"], c["board_h"], c["player_size"], c["projectile_size"]
    cov = dict(hit_p1=0, hit_p2=0, tick_limit_end=0, wall=[0, 0, 0, 0], edge=[0, 0, 0, 0], big_look_fire=0,
               far_apart=0, done_ticks=[])
    for t in range(tr.T):
        pre, raw, a = tr.pre[t], tr.raw[t], tr.actions[t].astype(np.float64)
        done, win = tr.done[t].astype(bool), tr.winner[t]
        cov["hit_p1"] += int((done & (win == 1)).sum())
        cov["hit_p2"] += int((done & (win == 2)).sum())
        cov["tick_limit_end"] += int((done & (win == 0)).sum())
        if done.any():
            cov["done_ticks"].append(t)
        live = ((pre["misc"][:, 1].view(np.uint32) >> 16) & 0xFF) != 0
        for p in (0, 1):
            x, y, r = pre["pos"][:, 2 * p], pre["pos"][:, 2 * p + 1], pre["rot"][:, p]
            s = np.clip(a[p, :, 0], -1.0, 1.0)
            nx = np.rint(x - np.sin(r) * c["player_speed"] * s)
            ny = np.rint(y - np.cos(r) * c["player_speed"] * s)
            stay = (raw["pos"][:, 2 * p] == x) & (raw["pos"][:, 2 * p + 1] == y)
            for w, out in enumerate((nx < 0, nx + ps > W, ny < 0, ny + ps > H)):
                cov["wall"][w] += int((out & stay).sum())
            # the projectile after shoot: fired from the post-move position with the post-look rotation, else in flight
            fires = pre["qcdage"][:, 2 * p] <= 0
            look = np.clip(a[p, :, 1], -1.0, 1.0) * c["look_speed"]
            cov["big_look_fire"] += int((fires & (np.abs(look) > math.pi / 4)).sum())
            was = (((pre["misc"][:, 1].view(np.uint32) >> (8 * p)) & 0xFF) != 0) | fires
            now = ((raw["misc"][:, 1].view(np.uint32) >> (8 * p)) & 0xFF) != 0
            qx = np.where(fires, raw["pos"][:, 2 * p], pre["qpos"][:, 2 * p])
            qy = np.where(fires, raw["pos"][:, 2 * p + 1], pre["qpos"][:, 2 * p + 1])
            qr = np.where(fires, r + look, pre["qrot"][:, p])
            mx = np.rint(qx - np.sin(qr) * c["projectile_speed"])
            my = np.rint(qy - np.cos(qr) * c["projectile_speed"])
            lost = live & was & ~now
            for w, out in enumerate((mx < 0, mx + qsz > W, my < 0, my + qsz > H)):
                cov["edge"][w] += int((out & lost).sum())
        if compared(t):
            st = tr.state[t]
            d = np.abs(st["pos"][:, [0, 1]].astype(np.int64) - st["pos"][:, [2, 3]])
            cov["far_apart"] += int((d > 46340).sum())
    return cov


def restarts_inside(tr, launch):
    """games that end at a tick which is not the last of its `launch`-tick launch"""
    return sum(int(tr.done[t].sum()) for t in range(tr.T) if (t + 1) % launch != 0)


# ---- comparisons
def assert_state_equal(got, want, where):
    """test_gpu_parity._assert_state_equal's rule: every field bit for bit (-0.0 == 0.0 aside)"""
    for k in ("pos", "rot", "qpos", "qrot", "qcdage", "misc"):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        same = ((g.view(np.int64) == w.view(np.int64)) | ((g == 0) & (w == 0))) if k in ("rot", "qrot") else g == w
        if not same.all():
            bad = np.argwhere(~same)
            raise AssertionError(f"{where}: {k} differs in {len(bad)} entries, first {bad[0]}: "
                                 f"{g[tuple(bad[0])]!r} vs {w[tuple(bad[0])]!r}")


def flag_mismatches_explained(cfg, state, got11, want11):
    """test_gpu_parity._flag_mismatches_explained at this configuration's player size: an obs[11] that
    differs from the oracle's (glibc tan) must be a projectile whose gradient glibc does not round
    correctly and whose flag the correctly rounded tan decides the device's way.  Returns their number."""
    from cr_tan import cr_tan
    ps = cfg["player_size"]
    bad = np.argwhere(got11 != want11)
    for p, i in bad:
        qx, qy = (int(v) for v in state["qpos"][i, 2 * p:2 * p + 2])
        ox, oy = (int(v) for v in state["pos"][i, 2 * (1 - p):2 * (1 - p) + 2])
        x = -float(state["qrot"][i, p]) + math.pi / 2
        g = cr_tan(x)
        assert math.tan(x) != g, (p, i)
        yi = float(qy) - g * float(qx)
        fut = any(float(oy) <= g * float(X) + yi <= float(oy + ps) for X in (ox, ox + ps))
        assert bool(got11[p, i]) == fut, (p, i)
    return len(bad)


def assert_close(got, want, where):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    if not (err <= OBS_TOL).all():  # (a NaN fails)
        bad = np.unravel_index(np.nanargmax(np.where(np.isnan(err), np.inf, err)), err.shape)
        raise AssertionError(f"{where}: err {err[bad]:.3g} at {bad}: got {got[bad]!r} want {want[bad]!r}")


def assert_obs(tr, state, got, want, where, exact_flag):
    """obs [2, n, 12] against the oracle's; state: the one the obs are of.  -> explained flag differences"""
    got = np.asarray(got, np.float64)
    assert_close(got[..., :11], want[..., :11], where)
    if exact_flag:
        assert np.array_equal(got[..., 11], want[..., 11]), f"{where}: obs[11]"
        return 0
    return flag_mismatches_explained(tr.cfg, state, got[..., 11], want[..., 11])


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _engine(ssa, tr, device):
    g = ssa.VecSkillshotGame(tr.n, device=device, seed=tr.seed, tick_limit=TICK_LIMIT, config=sk_config(tr.name))
    g.load_state_dict(tr.start)
    g.step_counter = tr.step0
    g.clear_counters()
    return g


def _state(g):
    st = g.state_dict()
    st.pop("step_counter")
    return st


def _finish(g, tr, explained, where):
    assert g.step_counter == tr.step_end, where
    c = g.counters()
    assert [c["dones"], c["hits_p1"], c["hits_p2"], c["ticks_sum"]] == tr.counters, where
    print(f"{where}: obs[11] differences explained by glibc's tan rounding: {explained}")
    return explained


def play(ssa, engine_kind, name, n, T, launch=1, reward="looking"):
    """Drive one engine path through configuration `name`'s oracle run and compare.

    engine_kind: "cpu" (the CPU backend, one step per tick), "step" (the GPU's one-tick kernel; the
    caller sets SK_STEP_VARIANT), "multi" (step_multi in launches of `launch` ticks; the caller sets the
    SK_MULTI_* knobs) or "multi_obs" (step_multi_obs, `reward` kind).  Actions must equal the oracle's
    draw.  State bit for bit on compared ticks (a multi launch: where they end a launch), done / winner
    every tick, counters and the RNG step counter at the end, obs / reward / obs_reset within OBS_TOL
    with obs[11] exact up to the flags cr_tan explains (the CPU backend: exact).
    """
    import torch
    tr = oracle_trace(name, n, T)
    cpu = engine_kind == "cpu"
    g = _engine(ssa, tr, "cpu" if cpu else "cuda")
    where = f"{name} {engine_kind} n={n} launch={launch}"
    explained = 0
    acts = g.gen_random_actions(T)
    assert np.array_equal(_np(acts), tr.actions), f"{where}: actions"
    if engine_kind in ("cpu", "step"):
        for t in range(T):
            cmp_ = compared(t)
            out = g.step(acts[t], obs=cmp_, reward=reward, auto_reset=True, reset_obs=cmp_)
            w = f"{where} t={t}"
            assert np.array_equal(_np(out["done"]), tr.done[t]), f"{w}: done"
            assert np.array_equal(_np(out["winner"]), tr.winner[t]), f"{w}: winner"
            if cmp_:
                assert_state_equal(_state(g), tr.state[t], w)
                explained += assert_obs(tr, tr.raw[t], _np(out["obs"]), tr.obs[t], w + " obs", cpu)
                explained += assert_obs(tr, tr.state[t], _np(out["obs_reset"]), tr.obs_reset[t], w + " obs_reset", cpu)
                assert_close(_np(out["reward"]), tr.reward_simple[t] if reward == "simple" else tr.reward[t],
                             w + " reward")
        return _finish(g, tr, explained, where)
    for t0 in range(0, T, launch):  # (the last launch is shorter where `launch` does not divide T)
        t1 = min(t0 + launch, T) - 1
        w = f"{where} ticks {t0}..{t1}"
        if engine_kind == "multi":
            done, winner = g.step_multi(acts[t0:t1 + 1], record=True, auto_reset=True)
            obs = rew = None
        else:
            out = g.step_multi_obs(acts[t0:t1 + 1], reward=reward, auto_reset=True)
            done, winner, obs, rew = out["done"], out["winner"], _np(out["obs"]), _np(out["reward"])
        if not cpu:
            torch.cuda.synchronize()
        assert np.array_equal(_np(done), np.stack(tr.done[t0:t1 + 1])), f"{w}: done"
        assert np.array_equal(_np(winner), np.stack(tr.winner[t0:t1 + 1])), f"{w}: winner"
        if compared(t1) or launch > 10:
            assert_state_equal(_state(g), tr.state[t1], w)
        for t in range(t0, t1 + 1):
            if obs is not None and compared(t):
                explained += assert_obs(tr, tr.raw[t], obs[t - t0], tr.obs[t], f"{w} obs t={t}", cpu)
                assert_close(rew[t - t0], tr.reward_simple[t] if reward == "simple" else tr.reward[t],
                             f"{w} reward t={t}")
    return _finish(g, tr, explained, where)
