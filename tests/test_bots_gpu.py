"""Scripted actors on the GPU: sk_env_bot_act against the CPU backend bit for
bit; the one-launch league with scripted seats (sk_env_act_league_bots, a
seat without an MFMA tile) against a per-tick loop, and SkillshotLearner's
league / evaluate fused against their loop paths, records included; a match
with a random seat played in two launches; the pool tick with a scripted
opponent (sk_env_act_step_pool_bots) against the composition; and the old
symbols still refusing a (0, kind) row."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GAMES, BLOCK, LIMIT = 40, 64, 64  # two workgroups per pairing, 24 pad games
ENV_SEED = 6
ACTOR_SEEDS = (23, 27)            # test_league_gpu's: they turn, move and hit
LIVE = 0x00FF0000
KINDS = ("still", "random", "aimer", "chaser")


@pytest.fixture(scope="module")
def kit():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import skillshot_learning_amd as ssa
    from skillshot_learning_amd import learner
    from skillshot_learning_amd.actor_kernel import ActorKernel32
    from skillshot_learning_amd.scripted import ScriptedActor
    from skillshot_learning_amd.vec_env import PLANES
    from test_match_cpu import turning_actor
    nets = [turning_actor(s).cuda() for s in ACTOR_SEEDS]
    kernels = [ActorKernel32(m, seed=5 + k) for k, m in enumerate(nets)]
    return dict(ssa=ssa, learner=learner, nets=nets, kernels=kernels, PLANES=PLANES, Bot=ScriptedActor)


def bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype != torch.bool else t


def planes_of(kit, g):
    return {name: getattr(g, name).clone() for name, _, _ in kit["PLANES"]}


# ---------------------------------------------------------------- 1. bot_actions
@pytest.mark.parametrize("name", [None, "cfg_packed"])
def test_bot_actions_equal_the_cpu_backend(kit, name):
    """N = 70: 140 lanes, a partial last workgroup"""
    import config_cases as cc
    cfg = cc.sk_config(name) if name else None
    n = 70
    envs = [kit["ssa"].VecSkillshotGame(n, device=d, seed=11, env_offset=5, tick_limit=60, config=cfg)
            for d in ("cpu", "cuda")]
    c, g = envs
    c.reset(random_positions=True)
    c.rollout_random(30)
    st = c.state_dict()
    st["rot"][3] = (1.0e7, -2.5e6)  # past sincos_bf's range: the library routine on both backends
    c.load_state_dict(st)
    g.load_state_dict(st)
    assert g.step_counter == c.step_counter
    for kind in KINDS:
        want, got = c.bot_actions(kind), g.bot_actions(kind)
        torch.cuda.synchronize()
        assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)), (name, kind)
    assert torch.equal(g.bot_actions("random"), g.gen_random_actions(1)[0])
    assert g.step_counter == c.step_counter
    for k, v in g.state_dict().items():
        assert np.array_equal(np.asarray(v), np.asarray(st[k])), k


# ---------------------------------------------------------------- 2. the league
def league_actors(kit):
    return [kit["kernels"][0], kit["Bot"]("chaser"), kit["Bot"]("random"), kit["Bot"]("aimer")]


PAIRS = [(i, j) for i in range(4) for j in range(4) if i != j]  # net/bot, bot/net and bot/bot


def start_of(kit):
    g = kit["ssa"].VecSkillshotGame(GAMES, device="cuda", seed=ENV_SEED, tick_limit=LIMIT)
    g.step_counter = 0
    g.reset(random_positions=True)
    return g, g.state_dict(), g.observe()[0].clone()


def league_env(kit, start, obs0, pairs):
    """test_league_gpu's league start: every block the GAMES start states, then pad games that are not live"""
    P = len(pairs)
    lg = kit["ssa"].VecSkillshotGame(P * BLOCK, device="cuda", seed=ENV_SEED, tick_limit=LIMIT)
    sd = {}
    for name, _, w in kit["PLANES"]:
        src = np.asarray(start[name]).reshape(GAMES, w)
        t = np.empty((P, BLOCK, w), dtype=src.dtype)
        t[:, :GAMES] = src[None]
        t[:, GAMES:] = src[0]
        if name == "misc":
            t[:, GAMES:, 1] &= ~LIVE
        sd[name] = t.reshape(P * BLOCK, w)
    sd["step_counter"] = start["step_counter"]
    lg.load_state_dict(sd)
    obs = torch.zeros((2, P, BLOCK, 12), device="cuda")
    obs[:, :, :GAMES] = obs0[:, None]
    return lg, sd, obs.view(2, P * BLOCK, 12)


def loop_pairing(kit, g, a1, a2, obs, reward):
    """one pairing tick by tick on env g, ended games frozen: (lengths, returns, newest obs); g holds the final states"""
    Bot = kit["Bot"]
    alive = g.game_live & (g.ticks < g.tick_limit)
    lengths = torch.zeros(g.n, dtype=torch.int32, device="cuda")
    ret = torch.zeros((2, g.n), device="cuda")
    obs = obs.clone()
    while bool(alive.any()):
        act = torch.stack([a.actions(g)[p] if isinstance(a, Bot) else a(obs[p]) for p, a in enumerate((a1, a2))])
        keep = planes_of(kit, g)
        out = g.step(act, obs=True, reward=reward, auto_reset=False)
        for name, t in keep.items():
            getattr(g, name).copy_(torch.where(alive[:, None], getattr(g, name), t))
        ret = torch.where(alive[None], ret + out["reward"], ret)
        lengths += alive.int()
        obs = torch.where(alive[None, :, None], out["obs"], obs)
        alive = alive & ~out["done"].bool()
    return lengths, ret, obs


@pytest.mark.parametrize("reward", ["looking", "simple"])
def test_league_with_scripted_seats_equals_the_loop(kit, monkeypatch, reward):
    """every pairing of a net and three scripted actors in one launch against
    the per-tick loop of each pairing on an env whose games carry the ids they
    have in the launch (the random policy's key): lengths, returns, newest
    observations and final planes, and the pad games untouched"""
    monkeypatch.setenv("SK_FWD16", "0")
    actors = league_actors(kit)
    ctr = int(kit["kernels"][0]._ctr[0])
    g, start, obs0 = start_of(kit)
    lg, sd, obs = league_env(kit, start, obs0, PAIRS)
    c0 = lg.step_counter
    m = lg.act_league(actors, PAIRS, BLOCK, obs, n_ticks=LIMIT, reward=reward)
    torch.cuda.synchronize()
    P = len(PAIRS)
    ln, ret, ob = m["lengths"].view(P, BLOCK), m["returns"].view(2, P, BLOCK), m["obs"].view(2, P, BLOCK, 12)
    T, hits = 0, 0
    for p, (i, j) in enumerate(PAIRS):
        gp = kit["ssa"].VecSkillshotGame(GAMES, device="cuda", seed=ENV_SEED, env_offset=p * BLOCK, tick_limit=LIMIT)
        gp.load_state_dict(start)
        wl, wr, wo = loop_pairing(kit, gp, actors[i], actors[j], obs0, reward)
        assert torch.equal(ln[p, :GAMES], wl), (p, i, j)
        assert torch.equal(bits(ret[:, p, :GAMES]), bits(wr)), (p, i, j)
        assert torch.equal(bits(ob[:, p, :GAMES]), bits(wo)), (p, i, j)
        for name, _, w in kit["PLANES"]:
            assert torch.equal(bits(getattr(lg, name).view(P, BLOCK, w)[p, :GAMES]), bits(getattr(gp, name))), (p, name)
        T = max(T, int(wl.max()))
        hits += int((gp.winner_id != 0).sum())
    assert lg.step_counter == c0 + T and T > 32
    print(f"{reward}: {hits} hits over the 12 pairings, longest game {T}")
    assert hits >= 40  # the chaser hits: equality must not pass on games that all run to the limit
    assert int(ln[:, GAMES:].abs().sum()) == 0 and int((ret[:, :, GAMES:] != 0).sum()) == 0
    for name, _, w in kit["PLANES"]:
        got = getattr(lg, name).view(P, BLOCK, w)[:, GAMES:]
        assert torch.equal(bits(got), bits(torch.as_tensor(sd[name]).view(P, BLOCK, w)[:, GAMES:].cuda())), name
    assert int(kit["kernels"][0]._ctr[0]) == ctr  # the net's noise call number stays


def gpu_learner(kit, seed=9):
    torch.manual_seed(seed)
    L = kit["learner"].SkillshotLearner(n_envs=64, device="cuda", seed=seed, tick_limit=40, precision="fp32")
    with torch.no_grad():
        L.model_actor.load_state_dict(kit["nets"][0].state_dict())
    return L


def assert_same_record(a, b):
    assert a.rows == b.rows and a.slabs == b.slabs and a.pairs == b.pairs
    assert torch.equal(a.lengths, b.lengths) and torch.equal(a.games, b.games)
    for name in a.states:
        assert torch.equal(bits(a.states[name]), bits(b.states[name])), name
    assert torch.equal(bits(a.actions), bits(b.actions)) and torch.equal(bits(a.rewards), bits(b.rewards))


def test_learner_league_fused_equals_the_loop_path(kit, monkeypatch):
    """SkillshotLearner.league with scripted entries: the one launch against
    the pair-by-pair per-tick loop (SK_LEAGUE_KERNEL=0, SK_MATCH_KERNEL=0): the
    tables, and with record=33 (across the workgroup boundary) every plane,
    action and reward of the record"""
    monkeypatch.setenv("SK_FWD16", "0")
    L = gpu_learner(kit)
    env = L.game_environment
    before, step, calls = env.state_dict(), env.step_counter, L.actor_kernel.calls
    actors = [None, "chaser", "random", "aimer"]
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("SK_LEAGUE_KERNEL", flag)
        monkeypatch.setenv("SK_MATCH_KERNEL", flag)
        res[flag] = L.league(actors, games=GAMES, tick_limit=LIMIT, seed=ENV_SEED, record=33)
    recs = [res[f].pop("record") for f in ("1", "0")]
    assert res["1"] == res["0"]
    assert recs[0].rows == 12 * 33
    assert_same_record(recs[0], recs[1])
    assert len(L._league_envs) == 1 and next(iter(L._league_envs.values())).n == 12 * BLOCK
    r = res["1"]
    print(r["seat_wins"], r["elo"], r["ranking"])
    assert sum(map(sum, r["seat_wins"])) + sum(map(sum, r["seat_losses"])) >= 40
    monkeypatch.setenv("SK_LEAGUE_KERNEL", "1")
    monkeypatch.setenv("SK_MATCH_KERNEL", "1")
    again = L.league(actors, games=GAMES, tick_limit=LIMIT, seed=ENV_SEED)
    assert again == r  # the same call plays the same games
    # nothing of training moved
    after = env.state_dict()
    for k in before:
        assert np.array_equal(np.asarray(before[k]), np.asarray(after[k])), k
    assert env.step_counter == step and L.actor_kernel.calls == calls


# ---------------------------------------------------------------- 3. evaluate
def test_evaluate_against_a_scripted_opponent_fused_equals_the_loop_path(kit, monkeypatch):
    monkeypatch.setenv("SK_FWD16", "0")
    L = gpu_learner(kit)
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("SK_MATCH_KERNEL", flag)
        res[flag] = L.evaluate("chaser", games=GAMES, tick_limit=LIMIT, seed=ENV_SEED, record=3)
    recs = [res[f].pop("records") for f in ("1", "0")]
    assert res["1"] == res["0"]
    print({k: v for k, v in res["1"].items() if k != "legs"})
    assert res["1"]["wins"] + res["1"]["losses"] >= 10 and res["1"]["games"] == 2 * GAMES
    assert len(recs[0]) == len(recs[1]) == 2
    for a, b in zip(*recs):
        assert a.rows == 3
        assert_same_record(a, b)
    # leg 2 seats the chaser first: its recorded seat-1 moves are 0 or 1
    assert set(recs[0][1].actions[:, 0, :, 0].unique().tolist()) <= {0.0, 1.0}


def test_random_seat_in_two_launches_equals_one(kit, monkeypatch):
    """a net against the random policy, 32 + 32 ticks with resume=True against
    one 64-tick launch: the step counter, the random policy's key, carries on"""
    monkeypatch.setenv("SK_FWD16", "0")
    actors, pairs = [kit["kernels"][0], kit["Bot"]("random")], [(0, 1), (1, 0)]
    g, start, obs0 = start_of(kit)
    out = []
    for chunks in ((LIMIT,), (32, 32)):
        lg, sd, obs = league_env(kit, start, obs0, pairs)
        c0 = lg.step_counter
        m = lg.act_league(actors, pairs, BLOCK, obs, n_ticks=chunks[0])
        for t in chunks[1:]:
            assert lg.step_counter == c0 + chunks[0]
            m = lg.act_league(actors, pairs, BLOCK, m["obs"], n_ticks=t, out=m, resume=True)
        torch.cuda.synchronize()
        out.append((m["lengths"].clone(), m["returns"].clone(), m["obs"].clone(), planes_of(kit, lg), lg.step_counter))
    (l1, r1, o1, p1, s1), (l2, r2, o2, p2, s2) = out
    assert int(l1.max()) > 40  # games live past the first launch
    assert torch.equal(l1, l2) and torch.equal(bits(r1), bits(r2)) and torch.equal(bits(o1), bits(o2)) and s1 == s2
    for name in p1:
        assert torch.equal(bits(p1[name]), bits(p2[name])), name


# ---------------------------------------------------------------- 4. the pool tick
@pytest.mark.parametrize("kind", ["chaser", "random"])
def test_pool_tick_with_a_scripted_opponent_equals_the_composition(kit, monkeypatch, kind):
    """256 games, the learner (parameter noise), a scripted opponent and a
    net: three ticks of one launch each against every net's forward plus
    bot_actions, a select by (seat, block), then step_insert"""
    monkeypatch.setenv("SK_FWD16", "0")
    n, sd_noise = 256, 0.5
    pairs = kit["learner"].pool_pairs(n, 2, self_play=1)
    bot = kit["Bot"](kind)
    actors = [kit["kernels"][0], bot, kit["kernels"][1]]
    seat = torch.tensor(pairs, device="cuda").t().repeat_interleave(32, dim=1)  # [2, N]
    runs = []
    for fused in (True, False):
        for k, kern in enumerate(kit["kernels"]):
            kern._ctr.zero_()
            kern._ctr[0] = 7 + 4 * k
        g = kit["ssa"].VecSkillshotGame(n, device="cuda", seed=ENV_SEED, tick_limit=25)
        g.step_counter = 0
        g.reset(random_positions=True)
        g.rollout_random(20)  # turned players, projectiles in flight, games about to end
        ring = kit["learner"].ReplayRing(2 * 2 * n + 5, "cuda")  # wraps inside the third tick
        obs = g.observe()[0].clone()
        per = []
        for _ in range(3):
            if fused:
                out = g.act_step_pool(actors, pairs, 32, obs, noisy=0, noise_sd=sd_noise, ring=ring)
            else:
                x = obs.reshape(-1, 12)
                act = bot.actions(g).clone()
                for k in (0, 2):
                    a = actors[k](x, noise_sd=sd_noise if k == 0 else 0.0).view(2, n, 2)
                    act = torch.where((seat == k)[:, :, None], a, act)
                act = act.contiguous()
                out = g.step_insert(act, obs, ring, auto_reset=True, reset_obs=True)
                out["actions"] = act
            per.append({k: out[k].clone() for k in ("actions", "obs", "reward", "done", "obs_reset")})
            obs = per[-1]["obs_reset"]
        torch.cuda.synchronize()
        runs.append(dict(per=per, planes=planes_of(kit, g), ring=ring.buf.clone(), total=(int(ring.total_t), ring.total),
                         step=g.step_counter, calls=[k.calls for k in kit["kernels"]], counters=g.counters()))
    a, b = runs
    for t, (x, y) in enumerate(zip(a["per"], b["per"])):
        for k in x:
            assert torch.equal(bits(x[k]), bits(y[k])), (kind, t, k)
    for name in a["planes"]:
        assert torch.equal(bits(a["planes"][name]), bits(b["planes"][name])), name
    assert torch.equal(bits(a["ring"]), bits(b["ring"])) and a["total"] == b["total"] == (3 * 2 * n, 3 * 2 * n)
    assert a["step"] == b["step"] and a["counters"] == b["counters"]
    assert a["calls"] == b["calls"] == [7 + 3, 11]  # the learner drew once per tick, the frozen net never
    assert a["counters"]["dones"] >= 1
    # the scripted seats' rows of the stored actions are the policy's
    first = a["per"][0]["actions"]
    if kind == "chaser":
        assert set(first[..., 0][seat == 1].unique().tolist()) <= {0.0, 1.0}
    with pytest.raises(ValueError):
        g.act_step_pool([bot, kit["kernels"][0]], [(0, 1)] * 8, 32, obs, noisy=0, noise_sd=sd_noise)


# ---------------------------------------------------------------- 5. the old symbols
def test_net_only_league_still_refuses_a_scripted_row(kit, monkeypatch):
    """sk_env_act_league given a (0, kind) row, written straight into the
    device table: a null address as before — that actor's pairings get lengths
    0 and nothing else of theirs is written; the other pairing plays"""
    monkeypatch.setenv("SK_FWD16", "0")
    pairs = [(0, 1), (1, 0), (0, 0)]
    g, start, obs0 = start_of(kit)
    lg, sd, obs = league_env(kit, start, obs0, pairs)
    m = lg.act_league(kit["kernels"], pairs, BLOCK, obs, n_ticks=LIMIT)  # nets alone: sk_env_act_league
    torch.cuda.synchronize()
    want = (m["lengths"].clone(), m["returns"].clone(), planes_of(kit, lg))
    lg.load_state_dict(sd)
    m["nets"][1, 0], m["nets"][1, 1] = 0, 4
    m["call_lengths"].fill_(-1)
    m = lg.act_league(kit["kernels"], pairs, BLOCK, obs, n_ticks=LIMIT, out=m)  # same host tables: no upload
    torch.cuda.synchronize()
    assert m["nets"][1].tolist() == [0, 4]
    P = len(pairs)
    ln, ret = m["lengths"].view(P, BLOCK), m["returns"].view(2, P, BLOCK)
    assert int(ln[:2].abs().sum()) == 0 and int((ret[:, :2] != 0).sum()) == 0
    assert torch.equal(ln[2], want[0].view(P, BLOCK)[2]) and int(ln[2].max()) > 0
    assert torch.equal(bits(ret[:, 2]), bits(want[1].view(2, P, BLOCK)[:, 2]))
    for name, _, w in kit["PLANES"]:
        got = getattr(lg, name).view(P, BLOCK, w)
        loaded = torch.as_tensor(sd[name]).view(P, BLOCK, w).cuda()
        assert torch.equal(bits(got[:2]), bits(loaded[:2])), name
        assert torch.equal(bits(got[2]), bits(want[2][name].view(P, BLOCK, w)[2])), name
