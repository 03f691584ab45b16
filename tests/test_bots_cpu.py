"""Scripted actors without a GPU: sk_env_bot_act on the CPU backend against
the plain-Python restatement (bot_ref.py) on rolled-out and directed states,
whole recorded games tick by tick (recorded action = the policy of the
recorded pre-tick state; the C oracle stepped with the recorded actions
reproduces the recorded next state), the Python API, and the ladder's sanity
(chaser beats still)."""
import numpy as np
import pytest
import torch

import bot_ref
import config_cases as cc
import skillshot_learning_amd as ssa
from oracle import oracle
from skillshot_learning_amd import _capi
from skillshot_learning_amd.scripted import ScriptedActor
from skillshot_learning_amd.vec_env import PLANES
from test_match_cpu import GAMES, LIMIT, cpu_learner

CONFIGS = (None, "cfg_packed")  # the reference's constants; every field different (look 0.4, player 7)


def make_env(name, n, seed=5, device="cpu"):
    return ssa.VecSkillshotGame(n, device=device, seed=seed, env_offset=3, tick_limit=60,
                                config=cc.sk_config(name) if name else None)


def ref_of(g, kind, pos=None, rot=None):
    c = g.config
    return bot_ref.actions(kind, g.pos.cpu().numpy() if pos is None else pos,
                           g.rot.cpu().numpy() if rot is None else rot, look_speed=c.look_speed,
                           player_size=c.player_size, seed=g.seed, env_offset=g.env_offset, step=g.step_counter)


# ---------------------------------------------------------------- 1. the policies
@pytest.mark.parametrize("name", CONFIGS)
def test_bot_actions_match_the_python_restatement_on_rolled_out_states(name):
    g = make_env(name, 64)
    g.reset(random_positions=True)
    g.rollout_random(30)
    step = g.step_counter
    before = g.state_dict()
    rnd = g.gen_random_actions(1)[0]
    for kind in bot_ref.KINDS:
        got = g.bot_actions(kind)
        assert got.shape == (2, 64, 2) and got.dtype == torch.float32
        bot_ref.assert_actions(kind, got.numpy(), ref_of(g, kind), f"{name} {kind}")
        assert torch.equal(g.bot_actions(_capi.__dict__["SK_BOT_" + kind.upper()]), got)  # by code
        assert torch.equal(ScriptedActor(kind).actions(g), got)
    assert torch.equal(g.bot_actions("still"), torch.zeros(2, 64, 2))
    assert torch.equal(g.bot_actions("random").view(torch.int32), rnd.view(torch.int32))
    look = g.bot_actions("aimer")[..., 1]
    assert float(look.abs().max()) <= 1.0 and len(torch.unique(look)) > 8  # clamped, and not all saturated
    # advances nothing
    after = g.state_dict()
    assert g.step_counter == step
    for k in before:
        assert np.array_equal(np.asarray(before[k]), np.asarray(after[k])), k


def directed_states(cfg):
    """(pos [N, 4], rot [N, 2], what seat 1 must do: (move of chaser, look) or None where only bot_ref decides)"""
    near = 8 * cfg.player_size
    ls = cfg.look_speed
    rows = [
        # rot = 0: a move goes by (0, -1), so the opponent straight behind is dx = 0, dy > 0: side = -0 dx = 0, look +1
        ((100, 50, 100, 50 + near + 9), (0.0, 0.0), (1.0, 1.0)),
        # ahead == 0 exactly (rot = 0, dy = 0): not in front, the sign of side = -dx decides
        ((100, 100, 100 + near + 1, 100), (0.0, 0.0), (1.0, -1.0)),
        ((100, 100, 100 - near - 1, 100), (0.0, 0.0), (1.0, 1.0)),
        # both players on one cell: side = ahead = 0 -> look +1, d2 = 0 -> no move
        ((77, 77, 77, 77), (0.3, -1.2), (0.0, 1.0)),
        # straight ahead (rot = 0, dy < 0, dx = 0): t = 0
        ((100, 120, 100, 20), (0.0, 0.0), (1.0, 0.0)),
        # saturated t: rot = 0, ahead = 10, side = -dx = 10 -> t = 1 / ls >= 1 for ls <= 1; the mirror image
        ((100, 100, 90, 90), (0.0, 0.0), (0.0 if 200 <= near * near else 1.0, 1.0 if ls <= 1 else 1.0 / ls)),
        ((100, 100, 110, 90), (0.0, 0.0), (0.0 if 200 <= near * near else 1.0, -1.0 if ls <= 1 else -1.0 / ls)),
        # d2 exactly near^2 (no move) and near^2 + 1 (move), on an axis and off it
        ((100, 100, 100, 100 - near), (0.0, 0.0), (0.0, 0.0)),
        ((100, 100, 101, 100 - near), (0.0, 0.0), (1.0, None)),
        # a generic state: only bot_ref decides
        ((30, 40, 120, 90), (2.5, -0.7), None),
    ]
    pos = np.array([r[0] for r in rows], np.int32)
    rot = np.array([r[1] for r in rows], np.float64)
    return pos, rot, [r[2] for r in rows]


@pytest.mark.parametrize("name", CONFIGS)
def test_bot_actions_on_directed_states(name):
    cfg = cc.sk_config(name) if name else _capi.default_config()
    pos, rot, want = directed_states(cfg)
    n = len(pos)
    g = make_env(name, n)
    st = g.state_dict()
    st["pos"], st["rot"] = pos, rot
    g.load_state_dict(st)
    aim, chase = g.bot_actions("aimer").numpy(), g.bot_actions("chaser").numpy()
    bot_ref.assert_actions("aimer", aim, ref_of(g, "aimer"), f"{name} aimer")
    bot_ref.assert_actions("chaser", chase, ref_of(g, "chaser"), f"{name} chaser")
    assert np.array_equal(aim[..., 0], np.zeros((2, n)))          # an aimer never moves
    assert np.array_equal(aim[..., 1], chase[..., 1])             # the same look
    for i, w in enumerate(want):
        if w is None:
            continue
        assert chase[0, i, 0] == w[0], (name, i, "move", chase[0, i])
        if w[1] is not None:
            assert abs(float(chase[0, i, 1]) - w[1]) <= bot_ref.LOOK_TOL, (name, i, "look", chase[0, i])
    # exactly behind at rot = 0 is the tie the tolerance excludes: it is +1 bit for bit, for both seats' geometry
    assert chase[0, 0, 1] == 1.0 and chase[0, 3, 1] == 1.0 and chase[1, 3, 1] == 1.0


def test_bad_kinds_and_buffers_are_refused():
    g = make_env(None, 8)
    for bad in ("runner", 0, 5, -1, None, 2.0, True):
        with pytest.raises(ValueError):
            g.bot_actions(bad)
        with pytest.raises(ValueError):
            ScriptedActor(bad)
    with pytest.raises(ValueError):
        g.bot_actions("still", out=torch.zeros(2, 8, 3))
    assert ScriptedActor("chaser").kind == _capi.SK_BOT_CHASER == 4 and ScriptedActor(3).name == "aimer"
    lib = ssa.load_library()
    buf = np.zeros(64, np.float32)
    for kind in (0, 5):
        assert lib.sk_env_bot_act(g._h, kind, buf.ctypes.data, None) == _capi.SK_EINVAL
    assert lib.sk_env_bot_act(g._h, 1, None, None) == _capi.SK_EINVAL
    assert lib.sk_env_bot_act(None, 1, buf.ctypes.data, None) == _capi.SK_EINVAL
    assert lib.sk_env_bot_act(g._h, 1, buf.ctypes.data + 4, None) == _capi.SK_EINVAL
    for name in ("sk_env_act_league_bots", "sk_env_act_league_bots_rec", "sk_env_act_step_pool_bots"):
        assert name in _capi.EXPORTS and getattr(lib, name) is not None


# ---------------------------------------------------------------- 2. whole games, tick by tick
def check_record(rec, kinds, seed, env_offset, first_step, shifts):
    """every recorded tick of every row: the scripted seats' recorded actions
    are bot_ref's of the recorded pre-tick state, and the C oracle stepped
    with the recorded actions gives the recorded next state exactly.  kinds[j]
    = (seat-1 kind, seat-2 kind) of row j, None for a net; shifts[j]: what the
    row's env adds to env_offset."""
    rec = rec.cpu()
    cfg = rec.config
    checked = 0
    for j in range(rec.rows):
        gm = rec.game(j)
        L, game = gm["length"], int(rec.games[j])
        assert L >= 1
        orc = oracle.OracleState(1, seed=seed, env_offset=env_offset + shifts[j] + game, config=cfg)
        for t in range(L):
            pre = {name: gm["states"][name][t].numpy() for name, _, _ in PLANES}
            for p, kind in enumerate(kinds[j]):
                if kind is None:
                    continue
                want = bot_ref.actions(kind, pre["pos"], pre["rot"], look_speed=cfg.look_speed,
                                       player_size=cfg.player_size, seed=seed,
                                       env_offset=env_offset + shifts[j] + game, step=first_step + t)
                bot_ref.assert_actions(kind, gm["actions"][t, p].numpy()[None], want[p], f"row {j} tick {t} seat {p + 1}")
                checked += 1
            orc.load({name: v[None] for name, v in pre.items()})
            orc.step(gm["actions"][t].numpy()[:, None, :], tick_limit=rec.slabs - 1, auto_reset=False)
            for name, _, _ in PLANES:
                assert np.array_equal(orc.arrays()[name][0], gm["states"][name][t + 1].numpy()), (j, t, name)
    return checked


def test_recorded_games_follow_the_policies_tick_by_tick():
    L = cpu_learner()
    env = L._eval_env(GAMES, LIMIT, None)
    res = L.evaluate("chaser", games=GAMES, tick_limit=LIMIT, record=8)
    assert len(res["records"]) == 2 and all(r.rows == 8 for r in res["records"])
    # the legs start at step 1: the evaluation env's reset took step 0
    n1 = check_record(res["records"][0], [(None, "chaser")] * 8, env.seed, env.env_offset, 1, [0] * 8)
    n2 = check_record(res["records"][1], [("chaser", None)] * 8, env.seed, env.env_offset, 1, [0] * 8)
    assert n1 >= 8 and n2 >= 8
    lg = L.league(["aimer", "random"], games=GAMES, tick_limit=LIMIT, record=4)
    rec = lg["record"]
    assert rec.rows == 8 and rec.pairs == [(0, 1)] * 4 + [(1, 0)] * 4
    block = 32 * ((GAMES + 31) // 32)
    n3 = check_record(rec, [("aimer", "random")] * 4 + [("random", "aimer")] * 4, env.seed, env.env_offset, 1,
                      [0] * 4 + [block] * 4)  # pairing 1's games carry the ids they have in the one launch
    assert n3 >= 16


# ---------------------------------------------------------------- 3. the API
def test_evaluate_league_train_vs_accept_scripted_actors_and_leave_training_alone():
    L = cpu_learner()
    L.model_train(1)  # a ring / counters with history
    env = L.game_environment
    before, step, gen, total = env.state_dict(), env.step_counter, L.gen.get_state().clone(), L.replay.total
    calls = getattr(L.actor_kernel, "calls", None)
    a = L.evaluate("chaser", games=GAMES, tick_limit=LIMIT)
    b = L.evaluate(ScriptedActor("chaser"), games=GAMES, tick_limit=LIMIT)
    assert a == b and a["games"] == 2 * GAMES and a["wins"] + a["losses"] + a["draws"] == a["games"]
    assert L.evaluate("random", games=GAMES, tick_limit=LIMIT) == L.evaluate(ScriptedActor(2), games=GAMES,
                                                                             tick_limit=LIMIT)
    l1 = L.league([None, "still", ScriptedActor("aimer"), "random"], games=16, tick_limit=LIMIT)
    l2 = L.league([None, "still", ScriptedActor("aimer"), "random"], games=16, tick_limit=LIMIT)
    assert l1 == l2 and l1["n_actors"] == 4
    sw, sl, sd = (np.array(l1[k]) for k in ("seat_wins", "seat_losses", "seat_draws"))
    assert np.array_equal((sw + sl + sd)[~np.eye(4, dtype=bool)], np.full(12, 16))
    for bad in ("runner", 2.5):
        with pytest.raises((ValueError, TypeError)):
            L.evaluate(bad, games=GAMES, tick_limit=LIMIT)
        with pytest.raises((ValueError, TypeError)):
            L.league([None, bad], games=16, tick_limit=LIMIT)
    after = env.state_dict()
    for k in before:
        assert np.array_equal(np.asarray(before[k]), np.asarray(after[k])), k
    assert env.step_counter == step and torch.equal(L.gen.get_state(), gen) and L.replay.total == total
    assert getattr(L.actor_kernel, "calls", None) == calls


def test_train_vs_scripted_opponents_fill_2n_rows_per_tick():
    torch.manual_seed(4)
    from skillshot_learning_amd.learner import SkillshotLearner
    L = SkillshotLearner(n_envs=64, device="cpu", seed=4, tick_limit=LIMIT, replay_capacity=4096)
    t0, s0 = L.replay.total, L.game_environment.step_counter
    L.train_vs(["chaser"], 3, batch=64, warmup=10 ** 9)
    assert L.replay.total - t0 == 3 * 2 * 64 and L.game_environment.step_counter == s0 + 3
    L.train_vs([ScriptedActor("random")], 1, batch=64, warmup=10 ** 9)
    assert L.replay.total - t0 == 4 * 2 * 64
    with pytest.raises((ValueError, TypeError)):
        L.train_vs(["runner"], 1)


# ---------------------------------------------------------------- 4. the ladder
def test_chaser_beats_still_from_either_seat():
    """64 random starts, limit 400: a chaser walks up to a still target and
    hits it; at least half of the games in each seating (a pure-Python
    simulation on its own starts gave 49 and 45 of 64)."""
    L = cpu_learner()
    lg = L.league(["chaser", "still"], games=64, tick_limit=400)
    seat1 = lg["seat_wins"][0][1]    # chaser in seat 1: player 2 (still) was hit
    seat2 = lg["seat_losses"][1][0]  # chaser in seat 2: player 1 (still) was hit
    print("chaser wins over still:", seat1, "of 64 in seat 1,", seat2, "of 64 in seat 2;",
          "losses", lg["seat_losses"][0][1], lg["seat_wins"][1][0])
    assert seat1 >= 32 and seat2 >= 32
    assert lg["ranking"][0] == 0
