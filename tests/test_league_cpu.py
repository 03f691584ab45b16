"""League evaluation without a GPU: SkillshotLearner.league on the CPU backend
(the pairings played one by one with evaluate's leg) against the pairwise
evaluate calls, its identities, what it must leave alone, checkpoint actors,
bad input, the Bradley-Terry fit, and sk_env_act_league's argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import skillshot_learning_amd as ssa
from skillshot_learning_amd import _capi
from skillshot_learning_amd.learner import Actor, bradley_terry_elo
from test_match_cpu import GAMES, LIMIT, cpu_learner, turning_actor

TABLES = ("seat_wins", "seat_losses", "seat_draws", "mean_ticks", "mean_return", "opponent_mean_return")


@pytest.fixture(scope="module")
def played():
    """one league of three actors and the three pairwise evaluates, shared (never modified)"""
    L = cpu_learner()
    B, C = turning_actor(12), turning_actor(13)
    res = L.league([None, B, C], games=GAMES, tick_limit=LIMIT)
    ev = {(0, 1): L.evaluate(opponent=B, games=GAMES, tick_limit=LIMIT),
          (0, 2): L.evaluate(opponent=C, games=GAMES, tick_limit=LIMIT)}
    with torch.no_grad():  # B against C: B becomes the learner's actor
        mine = {k: v.clone() for k, v in L.model_actor.state_dict().items()}
        L.model_actor.load_state_dict(B.state_dict())
    ev[(1, 2)] = L.evaluate(opponent=C, games=GAMES, tick_limit=LIMIT)
    with torch.no_grad():
        L.model_actor.load_state_dict(mine)
    return dict(L=L, B=B, C=C, league=res, evaluate=ev)


def close(a, b):
    return abs(a - b) <= 1e-9 * max(abs(a), abs(b))


def test_league_equals_pairwise_evaluate(played):
    r = played["league"]
    assert r["n_actors"] == 3 and r["games"] == GAMES
    hits = 0
    for (i, j), e in played["evaluate"].items():
        leg1, leg2 = e["legs"]  # i in seat 1 against j; then i in seat 2, j in seat 1
        assert (r["seat_wins"][i][j], r["seat_losses"][i][j], r["seat_draws"][i][j]) == \
            (leg1["wins"], leg1["losses"], leg1["draws"])
        assert r["mean_ticks"][i][j] == leg1["mean_ticks"]
        assert close(r["mean_return"][i][j], leg1["mean_return"])
        assert close(r["opponent_mean_return"][i][j], leg1["opponent_mean_return"])
        # [j][i]: j sits in seat 1, so leg 2's tallies with the roles renamed
        assert (r["seat_wins"][j][i], r["seat_losses"][j][i], r["seat_draws"][j][i]) == \
            (leg2["losses"], leg2["wins"], leg2["draws"])
        assert r["mean_ticks"][j][i] == leg2["mean_ticks"]
        assert close(r["mean_return"][j][i], leg2["opponent_mean_return"])
        assert close(r["opponent_mean_return"][j][i], leg2["mean_return"])
        assert r["wins"][i][j] == e["wins"] and r["wins"][j][i] == e["losses"]
        assert r["draws"][i][j] == r["draws"][j][i] == e["draws"]
        hits += e["wins"] + e["losses"]
    assert hits >= 6  # the pairings are not all draws
    for k in range(3):
        for t in TABLES:
            assert r[t][k][k] == 0


def test_league_identities(played):
    r, L = played["league"], played["L"]
    wins, draws = np.array(r["wins"]), np.array(r["draws"])
    off = ~np.eye(3, dtype=bool)
    assert ((wins + wins.T + draws)[off] == 2 * GAMES).all()
    sw, sl, sd = (np.array(r[k]) for k in ("seat_wins", "seat_losses", "seat_draws"))
    assert ((sw + sl + sd)[off] == GAMES).all()
    assert np.array_equal(wins, sw + sl.T) and np.array_equal(draws, sd + sd.T)
    score = (wins + 0.5 * draws).sum(1) / (4 * GAMES)
    assert np.allclose(r["score"], score, rtol=0, atol=1e-15)
    assert abs(sum(r["score"]) - 1.5) < 1e-12  # every game hands out one point
    assert sorted(r["ranking"]) == [0, 1, 2]
    elo = r["elo"]
    assert all(np.isfinite(elo)) and abs(sum(elo)) < 1e-6
    assert r["ranking"] == sorted(range(3), key=lambda i: (-elo[i], i))
    assert L.league([None, played["B"], played["C"]], games=GAMES, tick_limit=LIMIT) == r  # rewound: the same games
    two = L.league([None, played["B"]], games=GAMES, tick_limit=LIMIT)
    for t in TABLES:
        assert two[t][0][1] == r[t][0][1] and two[t][1][0] == r[t][1][0]


def test_league_leaves_training_state_alone():
    L = cpu_learner()
    L.model_train(1)  # a ring / counters with history
    env = L.game_environment
    before = env.state_dict()
    step, gen = env.step_counter, L.gen.get_state().clone()
    params = [p.detach().clone() for p in L.model_actor.parameters()]
    L.league([None, turning_actor(12), turning_actor(13)], games=GAMES, tick_limit=LIMIT)
    L.league([turning_actor(12), None], games=GAMES, tick_limit=LIMIT)
    after = env.state_dict()
    assert after.keys() == before.keys()
    for k in before:
        assert np.array_equal(np.asarray(before[k]), np.asarray(after[k])), k
    assert env.step_counter == step
    assert torch.equal(L.gen.get_state(), gen)
    for p, q in zip(L.model_actor.parameters(), params):
        assert torch.equal(p, q)


def test_league_of_checkpoints(tmp_path):
    L = cpu_learner()
    L.save_location = str(tmp_path / "training_models")
    saved = []
    for epoch, seed in ((1, 11), (2, 12), (3, 13)):
        with torch.no_grad():
            L.model_actor.load_state_dict(turning_actor(seed).state_dict())
        L.save_actor_critic_models(epoch)
        saved.append({k: v.clone() for k, v in L.model_actor.state_dict().items()})
    by_index = L.league([0, 1, 2], games=GAMES, tick_limit=LIMIT)
    modules = []
    for sd in saved:
        modules.append(Actor())
        modules[-1].load_state_dict(sd)
    assert L.league(modules, games=GAMES, tick_limit=LIMIT) == by_index
    assert L.league([saved[0], modules[1], None], games=GAMES, tick_limit=LIMIT) == by_index  # None: epoch 3's actor
    assert by_index["seat_wins"] != [[0] * 3] * 3
    with pytest.raises(ssa.SkillshotError):
        L.save_location = str(tmp_path / "nothing")
        L.league([0, 1], games=GAMES, tick_limit=LIMIT)


def test_league_refuses_bad_input():
    L = cpu_learner()
    for bad in ([], [None], [None] * 33, 5):
        with pytest.raises((TypeError, ValueError)):
            L.league(bad, games=GAMES, tick_limit=LIMIT)
    with pytest.raises((TypeError, ValueError)):
        L.league([None, "latest"], games=GAMES, tick_limit=LIMIT)
    with pytest.raises((TypeError, ValueError)):
        L.league([None, True], games=GAMES, tick_limit=LIMIT)


def test_league_holds_more_actors_than_evaluates_cache():
    """ten state_dicts: evaluate's 8-entry cache would drop the first two
    while the league still needs them; league's holder keeps all ten and
    evaluate's cache is not used"""
    L = cpu_learner()
    sds = [turning_actor(20 + k).state_dict() for k in range(10)]
    r = L.league(sds, games=4, tick_limit=10)
    assert r["n_actors"] == 10 and len(L._league_actors) == 10
    assert len({id(e["net"]) for e in L._league_actors.values()}) == 10
    assert not L.__dict__.get("_eval_opponents")
    L.league(sds[:2], games=4, tick_limit=10)
    assert len(L._league_actors) == 2  # the holder follows the latest league


def test_bradley_terry_elo_recovers_known_ratings():
    true = np.array([0.0, 100.0, 250.0, 400.0])
    n = np.where(np.eye(4, dtype=bool), 0.0, 1e6)
    expect = 1.0 / (1.0 + 10.0 ** ((true[None, :] - true[:, None]) / 400.0))  # E[i scores against j]
    elo = bradley_terry_elo(expect * n, n)
    print("elo", elo)
    for i in range(4):
        for j in range(4):
            assert abs((elo[i] - elo[j]) - (true[i] - true[j])) < 0.1
    assert abs(elo.mean()) < 1e-9


def test_bradley_terry_elo_keeps_an_unbeaten_actor_finite():
    n = np.where(np.eye(3, dtype=bool), 0.0, 20.0)
    score = np.array([[0.0, 20.0, 20.0], [0.0, 0.0, 12.0], [0.0, 8.0, 0.0]])  # actor 0 won everything
    elo = bradley_terry_elo(score, n)
    assert np.isfinite(elo).all() and elo[0] > elo[1] > elo[2]
    assert np.isfinite(bradley_terry_elo(np.zeros((2, 2)), np.zeros((2, 2)))).all()  # nothing played: 0, 0
    with pytest.raises(ValueError):
        bradley_terry_elo(np.zeros((2, 3)), np.zeros((2, 3)))


def test_act_league_refuses_the_cpu_backend_and_bad_arguments():
    """every sk_env_act_league argument check answers SK_EINVAL with its
    message before any launch; with every argument in order a CPU-backend
    handle is refused as such.  The ABI version is unchanged: the symbol is
    an addition."""
    lib = ssa.load_library()
    assert lib.sk_abi_version() == _capi.ABI_VERSION == 13
    h = ctypes.c_void_p()
    assert lib.sk_env_create(ctypes.byref(h), 64, 0, 7, -1, None) == _capi.SK_OK
    buf = (ctypes.c_float * 8192)()
    nets = (ctypes.c_uint64 * 4)()
    pairs = (ctypes.c_int32 * 4)(0, 1, 1, 0)
    ln = (ctypes.c_int32 * 64)()
    base = ctypes.addressof(buf)

    def call(env=h, nets=nets, n_actors=2, pairs=pairs, n_pairs=2, block=32, obs2=buf, returns=buf, lengths=ln,
             last_half=None, n_ticks=10):
        return lib.sk_env_act_league(env, nets, n_actors, pairs, n_pairs, block, obs2, returns, lengths, last_half,
                                     n_ticks, 0, 2000, None)

    def refused(word, **kw):
        assert call(**kw) == _capi.SK_EINVAL
        assert word in lib.sk_last_error(), (kw, lib.sk_last_error())

    refused(b"GPU")
    refused(b"table", nets=None)
    refused(b"table", pairs=None)
    refused(b"lengths", lengths=None)
    refused(b"obs2", obs2=None)
    refused(b"n_ticks", n_ticks=0)
    refused(b"n_actors", n_actors=0)
    refused(b"n_pairs", n_pairs=0)
    refused(b"block", block=0)
    refused(b"block", block=-32)
    refused(b"block", block=48, n_pairs=1)
    refused(b"n_pairs * block", n_pairs=3)
    refused(b"n_pairs * block", block=64)
    refused(b"aligned", nets=ctypes.c_void_p(ctypes.addressof(nets) + 4))
    refused(b"aligned", pairs=ctypes.c_void_p(ctypes.addressof(pairs) + 2))
    refused(b"aligned", lengths=ctypes.c_void_p(ctypes.addressof(ln) + 1))
    refused(b"aligned", returns=ctypes.c_void_p(base + 2))
    refused(b"aligned", obs2=ctypes.c_void_p(base + (8 if base % 16 == 0 else 16 - base % 16 + 8)))
    assert call(env=None) == _capi.SK_EINVAL
    assert lib.sk_env_destroy(h) == _capi.SK_OK
    g = ssa.VecSkillshotGame(64, device="cpu")
    with pytest.raises(ssa.SkillshotError):
        g.act_league([None, None], [(0, 1), (1, 0)], 32, g.observe()[0])
