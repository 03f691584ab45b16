"""Head-to-head evaluation without a GPU: the outcome rule (winner_id is the
id of the player who was HIT), SkillshotLearner.evaluate on the CPU backend
(the per-tick loop path), what it must leave alone, checkpoint opponents, and
sk_env_act_match's argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import skillshot_learning_amd as ssa
from skillshot_learning_amd import _capi
from skillshot_learning_amd.learner import Actor, SkillshotLearner, match_outcomes

GAMES, LIMIT = 48, 40


def turning_actor(seed):
    """an Actor whose policy actually turns and moves: l3.bias ~ N(0, 0.5)
    (with the default zero bias the outputs are near 0 and hardly any game
    ends by a hit)"""
    gen = torch.Generator().manual_seed(seed)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        a = Actor()
    with torch.no_grad():
        a.l3.bias.copy_(0.5 * torch.randn(2, generator=gen))
    return a


def cpu_learner(seed=3):
    torch.manual_seed(seed)
    L = SkillshotLearner(n_envs=8, device="cpu", seed=seed, tick_limit=LIMIT, replay_capacity=1024)
    with torch.no_grad():
        L.model_actor.load_state_dict(turning_actor(11).state_dict())
    return L


def test_match_outcomes_counts_the_hit_player_as_the_loser():
    w = np.array([0, 1, 2, 2, 1, 1, 0, 2, 2], dtype=np.uint8)  # 2 draws, 3 hits on seat 1, 4 on seat 2
    s1, s2 = match_outcomes(w, 1), match_outcomes(w, 2)
    assert s1 == dict(wins=4, losses=3, draws=2)   # seat 1 wins when player 2 was hit
    assert s2 == dict(wins=3, losses=4, draws=2)
    for seat in (1, 2):
        for wid in (0, 1, 2):
            o = match_outcomes([wid], seat)
            assert o["wins"] + o["losses"] + o["draws"] == 1
            assert o["losses"] == (wid == seat)          # a hit on the own seat is a loss, not a win
            assert o["wins"] == (wid == 3 - seat)
            assert o["draws"] == (wid == 0)
    t = match_outcomes(torch.as_tensor(w), 1)            # tensors: 0-d tensors, same counts
    assert {k: int(v) for k, v in t.items()} == s1
    assert sum(int(v) for v in t.values()) == len(w)
    with pytest.raises(ValueError):
        match_outcomes(w, 0)


def test_mirror_match_is_symmetric():
    L = cpu_learner()
    r = L.evaluate(opponent=None, games=GAMES, tick_limit=LIMIT, swap_sides=True)
    assert r["games"] == 2 * GAMES and r["wins"] + r["losses"] + r["draws"] == r["games"]
    # the legs are the same games with the roles renamed
    assert r["wins"] == r["losses"]
    a, b = r["legs"]
    assert (a["seat"], b["seat"]) == (1, 2) and a["games"] == b["games"] == GAMES
    assert a["wins"] == b["losses"] and a["losses"] == b["wins"] and a["draws"] == b["draws"]
    assert a["mean_ticks"] == b["mean_ticks"]
    assert a["mean_return"] == b["opponent_mean_return"] and a["opponent_mean_return"] == b["mean_return"]
    assert abs(r["win_rate"] + r["loss_rate"] + r["draw_rate"] - 1.0) < 1e-12
    for leg in r["legs"]:
        assert abs(leg["win_rate"] + leg["loss_rate"] + leg["draw_rate"] - 1.0) < 1e-12
    assert 0 < r["mean_ticks"] <= LIMIT
    assert L.evaluate(opponent=None, games=GAMES, tick_limit=LIMIT) == r  # rewound: the same games again
    one = L.evaluate(opponent=None, games=GAMES, tick_limit=LIMIT, swap_sides=False)
    assert len(one["legs"]) == 1 and {k: v for k, v in one["legs"][0].items() if k != "seat"} == \
        {k: v for k, v in a.items() if k != "seat"}


def test_different_opponent_is_seated_where_evaluate_says():
    """leg 1 has the learner in seat 1: against a different net the leg equals
    a hand-driven loop with the learner's actor on player 1's rows"""
    L = cpu_learner()
    opp = turning_actor(12)
    r = L.evaluate(opponent=opp, games=GAMES, tick_limit=LIMIT, swap_sides=False, reward="simple")
    g = ssa.VecSkillshotGame(GAMES, device="cpu", seed=L._eval_env(GAMES, LIMIT, None).seed, tick_limit=LIMIT)
    g.step_counter = 0
    g.reset(random_positions=True)
    obs, _ = g.observe()
    alive = torch.ones(GAMES, dtype=torch.bool)
    winner = torch.zeros(GAMES, dtype=torch.uint8)
    acc = torch.zeros(2, GAMES)
    with torch.no_grad():
        while bool(alive.any()):
            out = g.step(torch.stack((L.model_actor(obs[0]), opp(obs[1]))), reward="simple", auto_reset=False)
            acc = torch.where(alive[None], acc + out["reward"], acc)
            done = out["done"].bool()
            winner = torch.where(alive & done, out["winner"], winner)
            alive &= ~done
            obs = out["obs"]
    assert r["wins"] == int((winner == 2).sum()) and r["losses"] == int((winner == 1).sum())
    assert r["draws"] == int((winner == 0).sum())
    assert r["mean_return"] == float(acc[0].sum().double()) / GAMES
    assert r["opponent_mean_return"] == float(acc[1].sum().double()) / GAMES


def test_evaluate_leaves_training_state_alone():
    L = cpu_learner()
    L.model_train(1)  # a ring / counters with history
    env = L.game_environment
    before = env.state_dict()
    step, gen = env.step_counter, L.gen.get_state().clone()
    params = [p.detach().clone() for p in L.model_actor.parameters()]
    L.evaluate(opponent=turning_actor(12), games=GAMES, tick_limit=LIMIT)
    L.evaluate(opponent=None, games=GAMES, tick_limit=LIMIT)
    after = env.state_dict()
    assert after.keys() == before.keys()
    for k in before:
        assert np.array_equal(np.asarray(before[k]), np.asarray(after[k])), k
    assert env.step_counter == step
    assert torch.equal(L.gen.get_state(), gen)
    for p, q in zip(L.model_actor.parameters(), params):
        assert torch.equal(p, q)


def test_checkpoint_opponent(tmp_path):
    L = cpu_learner()
    L.save_location = str(tmp_path / "training_models")
    L.save_actor_critic_models(1)
    saved = {k: v.clone() for k, v in L.model_actor.state_dict().items()}
    with torch.no_grad():  # the learner moves on
        L.model_actor.load_state_dict(turning_actor(13).state_dict())
    actor_now = [p.detach().clone() for p in L.model_actor.parameters()]
    critic_now = [p.detach().clone() for p in L.model_critic.parameters()]
    by_index = L.evaluate(opponent=0, games=GAMES, tick_limit=LIMIT)
    module = Actor()
    module.load_state_dict(saved)
    assert L.evaluate(opponent=module, games=GAMES, tick_limit=LIMIT) == by_index
    assert L.evaluate(opponent=saved, games=GAMES, tick_limit=LIMIT) == by_index      # a state_dict
    assert L.evaluate(opponent=-1, games=GAMES, tick_limit=LIMIT) == by_index         # the only file
    assert by_index != L.evaluate(opponent=None, games=GAMES, tick_limit=LIMIT)
    for p, q in zip(L.model_actor.parameters(), actor_now):
        assert torch.equal(p, q)
    for p, q in zip(L.model_critic.parameters(), critic_now):
        assert torch.equal(p, q)
    with pytest.raises(ssa.SkillshotError):
        L.save_location = str(tmp_path / "nothing")
        L.evaluate(opponent=0, games=GAMES, tick_limit=LIMIT)
    with pytest.raises(TypeError):
        L.evaluate(opponent="latest", games=GAMES, tick_limit=LIMIT)


def test_act_match_refuses_the_cpu_backend_and_bad_arguments():
    """sk_env_act_match is GPU-only (the fused actors): SK_EINVAL with a
    message on a CPU-backend handle, and NULL lengths / n_ticks = 0 are
    SK_EINVAL (all checked before any launch)"""
    lib = ssa.load_library()
    assert lib.sk_abi_version() == _capi.ABI_VERSION == 13
    h = ctypes.c_void_p()
    assert lib.sk_env_create(ctypes.byref(h), 8, 0, 7, -1, None) == _capi.SK_OK
    buf = (ctypes.c_float * 4096)()
    ln = (ctypes.c_int32 * 8)()
    rc = lib.sk_env_act_match(h, buf, buf, buf, buf, buf, buf, ln, None, 10, 0, 2000, None)
    assert rc == _capi.SK_EINVAL and b"GPU" in lib.sk_last_error() and len(lib.sk_last_error()) > 0
    assert lib.sk_env_act_match(h, buf, buf, buf, buf, buf, buf, None, None, 10, 0, 2000, None) == _capi.SK_EINVAL
    assert b"lengths" in lib.sk_last_error()
    assert lib.sk_env_act_match(h, buf, buf, buf, buf, buf, buf, ln, None, 0, 0, 2000, None) == _capi.SK_EINVAL
    assert b"n_ticks" in lib.sk_last_error()
    # two faults: a bad argument is reported ahead of the CPU backend (as sk_env_act_league does)
    odd = ctypes.c_void_p(ctypes.addressof(ln) + 1)
    assert lib.sk_env_act_match(h, buf, buf, buf, buf, buf, buf, odd, None, 10, 0, 2000, None) == _capi.SK_EINVAL
    assert b"aligned" in lib.sk_last_error() and b"GPU" not in lib.sk_last_error()
    pack8 = ctypes.c_void_p(ctypes.addressof(buf) + 8)
    assert lib.sk_env_act_match(h, buf, buf, buf, pack8, buf, buf, ln, None, 10, 0, 2000, None) == _capi.SK_EINVAL
    assert b"aligned" in lib.sk_last_error() and b"GPU" not in lib.sk_last_error()
    assert lib.sk_env_act_match(None, buf, buf, buf, buf, buf, buf, ln, None, 10, 0, 2000, None) == _capi.SK_EINVAL
    assert lib.sk_env_destroy(h) == _capi.SK_OK
    g = ssa.VecSkillshotGame(4, device="cpu")
    with pytest.raises(ssa.SkillshotError):
        g.act_match(None, None, g.observe()[0])
