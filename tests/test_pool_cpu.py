"""Opponent-pool training without a GPU: sk_env_act_step_pool's argument
checks, the seating pool_pairs lays out, and SkillshotLearner.train_vs on the
CPU backend (the loop path: every actor's forward, a select by seat and block,
step and replay.add) read back from the replay ring."""
import ctypes

import pytest
import torch

import skillshot_learning_amd as ssa
from skillshot_learning_amd import _capi
from skillshot_learning_amd.learner import SkillshotLearner, pool_pairs
from test_match_cpu import turning_actor

LIMIT, TICKS = 25, 30
# the seeds were chosen on this loop path (CPU backend): over the 30 ticks the
# 128 games end 8 times by a hit (5 on player 1, 3 on player 2) and 122 times
# at the tick limit (every game not hit by tick 25 ends there), so games
# restart inside the run; the test asks for most of both
LEARNER_SEED, ACTOR_SEEDS = 5, (41, 42, 43)
ENDS_HIT, ENDS_LIMIT = 6, 110


def test_act_step_pool_refuses_the_cpu_backend_and_bad_arguments():
    """every sk_env_act_step_pool argument check answers SK_EINVAL with its
    message before any launch; with every argument in order a CPU-backend
    handle is refused as such.  The ABI version is unchanged: the symbol is an
    addition."""
    lib = ssa.load_library()
    assert lib.sk_abi_version() == _capi.ABI_VERSION == 13
    assert "sk_env_act_step_pool" in _capi.EXPORTS
    h = ctypes.c_void_p()
    assert lib.sk_env_create(ctypes.byref(h), 64, 0, 7, -1, None) == _capi.SK_OK
    buf = (ctypes.c_float * 8192)()
    ring = (ctypes.c_float * (28 * 160 + 8))()
    nets = (ctypes.c_uint64 * 4)()
    pairs = (ctypes.c_int32 * 4)(0, 1, 1, 0)
    ctr = (ctypes.c_uint64 * 130)()
    total = (ctypes.c_int64 * 2)()
    arrivals = (ctypes.c_uint32 * 288)()

    def aligned(arr, to=16):
        a = ctypes.addressof(arr)
        return a + (-a) % to

    obs_p, ring_p = aligned(buf), aligned(ring)

    def call(env=h, nets=nets, n_actors=2, pairs=pairs, n_pairs=2, block=32, noisy=0, acting_obs=obs_p,
             actions=obs_p, ctr=ctr, obs=obs_p, reward=obs_p, reward_kind=0, obs_reset=None, ring=None, capacity=0,
             total=None, arrivals=None, total_copy=None):
        P = ctypes.c_void_p
        return lib.sk_env_act_step_pool(env, nets, n_actors, pairs, n_pairs, block, noisy, P(acting_obs) if
                                        isinstance(acting_obs, int) else acting_obs, P(actions) if
                                        isinstance(actions, int) else actions, 0.5, 0.0, 9, ctr,
                                        P(obs) if isinstance(obs, int) else obs,
                                        P(reward) if isinstance(reward, int) else reward, reward_kind, None, None,
                                        LIMIT, 1, 1, P(obs_reset) if isinstance(obs_reset, int) else obs_reset,
                                        P(ring) if isinstance(ring, int) else ring, capacity, total, arrivals,
                                        P(total_copy) if isinstance(total_copy, int) else total_copy, None)

    def refused(word, **kw):
        assert call(**kw) == _capi.SK_EINVAL
        assert word in lib.sk_last_error(), (kw, lib.sk_last_error())

    refused(b"GPU")
    refused(b"GPU", ring=ring_p, capacity=160, total=total, arrivals=arrivals)  # every ring argument in order
    refused(b"table", nets=None)
    refused(b"table", pairs=None)
    refused(b"acting_obs", acting_obs=None)
    refused(b"actions", actions=None)
    refused(b"n_actors", n_actors=0)
    refused(b"n_pairs", n_pairs=0)
    refused(b"block", block=0)
    refused(b"block", block=-32)
    refused(b"block", block=48, n_pairs=1)
    refused(b"n_pairs * block", n_pairs=3)
    refused(b"n_pairs * block", block=64)
    refused(b"noisy_actor", noisy=2)
    refused(b"noisy_actor", noisy=-2)
    assert call(noisy=-1) == _capi.SK_EINVAL and b"GPU" in lib.sk_last_error()  # -1: nobody draws; in order
    refused(b"aligned", nets=ctypes.c_void_p(ctypes.addressof(nets) + 4))
    refused(b"aligned", pairs=ctypes.c_void_p(ctypes.addressof(pairs) + 2))
    refused(b"aligned", actions=obs_p + 4)
    refused(b"aligned", acting_obs=obs_p + 8)
    refused(b"aligned", ctr=ctypes.c_void_p(ctypes.addressof(ctr) + 4))
    refused(b"aligned", obs=obs_p + 8)
    refused(b"aligned", obs_reset=obs_p + 8)
    # sk_env_act_step's own checks (act_step_args)
    refused(b"reward_kind", reward_kind=2)
    refused(b"ring insert needs", ring=ring_p, capacity=160, total=None, arrivals=arrivals)
    refused(b"ring insert needs", ring=ring_p, capacity=160, total=total, arrivals=None)
    refused(b"ring insert needs", ring=ring_p, capacity=160, total=total, arrivals=arrivals, obs=None)
    refused(b"ring insert needs", ring=ring_p, capacity=160, total=total, arrivals=arrivals, reward=None)
    refused(b"capacity", ring=ring_p, capacity=127, total=total, arrivals=arrivals)
    refused(b"aligned", ring=ring_p + 4, capacity=160, total=total, arrivals=arrivals)
    refused(b"aligned", ring=ring_p, capacity=160, total=ctypes.c_void_p(ctypes.addressof(total) + 4),
            arrivals=arrivals)
    refused(b"aligned", ring=ring_p, capacity=160, total=total, arrivals=arrivals,
            total_copy=ctypes.addressof(total) + 4)
    assert call(env=None) == _capi.SK_EINVAL
    assert lib.sk_env_destroy(h) == _capi.SK_OK
    g = ssa.VecSkillshotGame(64, device="cpu")
    with pytest.raises(ssa.SkillshotError):
        g.act_step_pool([None, None], [(0, 1), (1, 0)], 32, g.observe()[0])


def test_pool_pairs_lists():
    assert pool_pairs(64, 1, 0) == [(0, 1), (1, 0)]
    assert pool_pairs(128, 1, 0) == [(0, 1), (1, 0), (0, 1), (1, 0)]
    assert pool_pairs(192, 2, 2) == [(0, 1), (1, 0), (0, 2), (2, 0), (0, 0), (0, 0)]
    assert pool_pairs(320, 2, 1) == [(0, 1), (1, 0), (0, 2), (2, 0), (0, 0)] * 2  # the cycle starts over
    assert pool_pairs(64, 1) == pool_pairs(64, 1, 0)
    with pytest.raises(ValueError):
        pool_pairs(48, 1, 0)  # no multiple of 32
    with pytest.raises(ValueError):
        pool_pairs(64, 2, 0)  # two blocks, a cycle of four
    with pytest.raises(ValueError):
        pool_pairs(96, 2, 2)
    with pytest.raises(ValueError):
        pool_pairs(64, 0, 0)
    with pytest.raises(ValueError):
        pool_pairs(0, 1, 0)


def pool_learner(n_envs, **kw):
    torch.manual_seed(LEARNER_SEED)
    L = SkillshotLearner(n_envs=n_envs, device="cpu", seed=LEARNER_SEED, tick_limit=LIMIT, replay_capacity=8192,
                         **kw)
    with torch.no_grad():
        L.model_actor.load_state_dict(turning_actor(ACTOR_SEEDS[0]).state_dict())
    return L


def test_train_vs_fills_the_ring_with_each_seat_s_own_actor():
    """30 ticks against two opponents at tick limit 25, no update (warmup
    beyond reach).  pool_pairs seats two opponents in both seats from four
    blocks on, so the run has 128 games, the fewest that hold the two
    (64 games, one cycle short, are refused), and the ring 30 * 256 rows: an
    opponent's rows hold exactly its forward of the stored state, the
    learner's rows its noisy action, and the opponents' nets are as given."""
    n = 128
    with pytest.raises(ValueError):
        pool_learner(64).train_vs([turning_actor(ACTOR_SEEDS[1]), turning_actor(ACTOR_SEEDS[2])], 1)
    L = pool_learner(n)
    opp = [turning_actor(s) for s in ACTOR_SEEDS[1:]]
    before = [{k: v.clone() for k, v in o.state_dict().items()} for o in opp]
    mine = {k: v.clone() for k, v in L.model_actor.state_dict().items()}
    c0 = L.game_environment.step_counter
    stats = L.train_vs(opp, TICKS, warmup=1 << 30)
    assert stats == [] and L.replay.total == TICKS * 2 * n == L.replay.size and int(L.replay.total_t) == L.replay.total
    assert L.game_environment.step_counter == c0 + TICKS
    for o, b in zip(opp, before):
        assert all(torch.equal(v, b[k]) for k, v in o.state_dict().items())
    assert all(torch.equal(v, mine[k]) for k, v in L.model_actor.state_dict().items())  # no update ran
    pairs = pool_pairs(n, 2, 0)
    assert pairs == [(0, 1), (1, 0), (0, 2), (2, 0)]
    seat = torch.tensor(pairs).t().repeat_interleave(32, dim=1)  # [2, N]: the actor of each (player, game)
    rows = L.replay.buf[:TICKS * 2 * n].view(TICKS, 2, n, 28)
    s, a = rows[..., :12], rows[..., 12:14]
    with torch.no_grad():
        for k, o in enumerate(opp):
            m = seat == k + 1
            assert int(m.sum()) == 64
            for t in range(TICKS):  # the forward on the whole observation, as the loop path calls it
                assert torch.equal(a[t][m], o(s[t].reshape(-1, 12)).view(2, n, 2)[m]), (k, t)
        m = seat == 0
        own = L.model_actor(s.reshape(-1, 12)).view(TICKS, 2, n, 2)[:, m]
        differ = (a[:, m] != own).any(-1)
        assert bool(differ.all())  # parameter noise was drawn for every learner row
    c = L.game_environment.counters()
    hits, limit = c["hits_p1"] + c["hits_p2"], c["dones"] - c["hits_p1"] - c["hits_p2"]
    print(f"game ends: {hits} by a hit, {limit} at the tick limit; done flags in the ring "
          f"{int(rows[:, 0, :, 27].sum())}")
    assert int(rows[:, 0, :, 27].sum()) == int(rows[:, 1, :, 27].sum()) == c["dones"]
    assert hits >= ENDS_HIT and limit >= ENDS_LIMIT
    # games restarted inside the run: a row after a done row starts from a fresh game's observation
    d = rows[:-1, 0, :, 27].bool()
    assert bool((rows[1:, 0, :, :12][d] != rows[:-1, 0, :, 14:26][d]).any())


def test_train_vs_updates_the_learner_and_mixes_with_train_ticks():
    """with warmup 0 the updates run and the actor changes; the opponents stay
    as given; train_ticks carries on from where train_vs left the env"""
    L = pool_learner(64)
    opp = turning_actor(ACTOR_SEEDS[1])
    before = {k: v.clone() for k, v in opp.state_dict().items()}
    mine = {k: v.clone() for k, v in L.model_actor.state_dict().items()}
    stats = L.train_vs([opp], 3, batch=32, warmup=0)
    assert len(stats) == 3 and L.replay.total == 3 * 128
    assert any(not torch.equal(v, mine[k]) for k, v in L.model_actor.state_dict().items())
    assert all(torch.equal(v, before[k]) for k, v in opp.state_dict().items())
    c0 = L.game_environment.step_counter
    assert len(L.train_ticks(2, batch=32, warmup=0)) == 2
    assert len(L.train_vs([opp], 2, batch=32, warmup=0)) == 2
    assert L.game_environment.step_counter == c0 + 4 and L.replay.total == 7 * 128
