"""League evaluation on the GPU: one sk_env_act_league launch (k_act_league32:
every pairing of K actors side by side, each workgroup reading its pairing's
two nets through device tables) against the launch it is built from,
sk_env_act_match on a `games`-game env with the same start, bit for bit; the
league played in chunks and under graph capture; the guard on a pair index
outside the table; and SkillshotLearner.league's two paths, its agreement with
pairwise evaluate, and its promise to leave training alone."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LIMIT = 60
ENV_SEED = 6
# seed 27 chosen on the CPU loop path: at 37 games each of the six off-diagonal
# pairings has at least 2 hits and a game shorter than 50 ticks, 16 hits in all
ACTOR_SEEDS = (23, 24, 27)
PAIRS = [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1), (0, 0)]  # the six ordered pairings and a mirror
LIVE = 0x00FF0000  # misc[:, 1] bits 16-23: game_live


@pytest.fixture(scope="module")
def kit():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import skillshot_learning_amd as ssa
    from skillshot_learning_amd import learner
    from skillshot_learning_amd.actor_kernel import ActorKernel32
    from skillshot_learning_amd.vec_env import PLANES
    from test_match_cpu import turning_actor
    nets = [turning_actor(s).cuda() for s in ACTOR_SEEDS]
    kernels = [ActorKernel32(m, seed=5 + k) for k, m in enumerate(nets)]
    for k, kern in enumerate(kernels):
        kern._ctr[0] = 7 + 4 * k  # noise call numbers with a history: a league must not move them
    return dict(ssa=ssa, learner=learner, nets=nets, kernels=kernels, PLANES=PLANES)


def bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype != torch.bool else t


_REFS = {}


def match_reference(kit, games, reward):
    """the parent's kernel, once per case (shared, never modified): the start
    of a `games`-game env and, per pairing, act_match's lengths, returns,
    final planes and observations from that start"""
    key = (games, reward)
    if key in _REFS:
        return _REFS[key]
    g = kit["ssa"].VecSkillshotGame(games, device="cuda", seed=ENV_SEED, tick_limit=LIMIT)
    g.step_counter = 0
    g.reset(random_positions=True)
    start = g.state_dict()
    obs0 = g.observe()[0].clone()
    per = []
    for i, j in PAIRS:
        g.load_state_dict(start)
        m = g.act_match(kit["kernels"][i], kit["kernels"][j], obs0, n_ticks=LIMIT, reward=reward)
        torch.cuda.synchronize()
        per.append(dict(lengths=m["lengths"].clone(), returns=m["returns"].clone(), obs=m["obs"].clone(),
                        planes={name: getattr(g, name).clone() for name, _, _ in kit["PLANES"]}))
    _REFS[key] = dict(start=start, obs0=obs0, per=per)
    return _REFS[key]


def league_start(kit, ref, games, block):
    """the league env's start: every block holds the `games` start states and
    then pad games, copies of game 0 with the live byte cleared; (state_dict,
    observations [2, P block, 12] with zero pad rows)"""
    P = len(PAIRS)
    sd = {}
    for name, _, w in kit["PLANES"]:
        src = np.asarray(ref["start"][name]).reshape(games, w)
        t = np.empty((P, block, w), dtype=src.dtype)
        t[:, :games] = src[None]
        t[:, games:] = src[0]
        if name == "misc":
            t[:, games:, 1] &= ~LIVE
        sd[name] = t.reshape(P * block, w)
    sd["step_counter"] = 0
    obs = torch.zeros((2, P, block, 12), device="cuda")
    obs[:, :, :games] = ref["obs0"][:, None]
    return sd, obs.view(2, P * block, 12)


def league_env(kit, ref, games, block):
    lg = kit["ssa"].VecSkillshotGame(len(PAIRS) * block, device="cuda", seed=ENV_SEED, tick_limit=LIMIT)
    sd, obs = league_start(kit, ref, games, block)
    lg.load_state_dict(sd)
    return lg, sd, obs


def assert_same_league(kit, lg, m, ref, sd, games, block, skip=()):
    """pairing p's games equal act_match's, the pad games are as loaded"""
    P = len(PAIRS)
    ln = m["lengths"].view(P, block)
    ret = m["returns"].view(2, P, block)
    obs = m["obs"].view(2, P, block, 12)
    for p in range(P):
        if p in skip:
            continue
        r = ref["per"][p]
        assert torch.equal(ln[p, :games], r["lengths"]), p
        assert torch.equal(bits(ret[:, p, :games]), bits(r["returns"])), p
        assert torch.equal(bits(obs[:, p, :games]), bits(r["obs"])), p
        for name, _, w in kit["PLANES"]:
            got = getattr(lg, name).view(P, block, w)[p, :games]
            assert torch.equal(bits(got), bits(r["planes"][name])), (p, name)
    assert int(ln[:, games:].abs().sum()) == 0
    assert int((ret[:, :, games:] != 0).sum()) == 0
    for name, dt, w in kit["PLANES"]:
        got = getattr(lg, name).view(P, block, w)[:, games:]
        want = torch.as_tensor(sd[name]).view(P, block, w)[:, games:].cuda()
        assert torch.equal(bits(got), bits(want)), name


@pytest.mark.parametrize("reward", ["looking", "simple"])
@pytest.mark.parametrize("games,block", [(37, 64), (32, 32), (1, 32)])
def test_act_league_equals_act_match(kit, monkeypatch, games, block, reward):
    """37 games in blocks of 64: two workgroups per pairing, a tail of 5 and
    27 pad games; 32 in 32: no pad; 1 in 32: 31 pad games"""
    monkeypatch.setenv("SK_FWD16", "0")
    ref = match_reference(kit, games, reward)
    ctrs = [int(k._ctr[0]) for k in kit["kernels"]]
    lg, sd, obs = league_env(kit, ref, games, block)
    c0 = lg.step_counter
    half = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    m = lg.act_league(kit["kernels"], PAIRS, block, obs, n_ticks=LIMIT, reward=reward, out=dict(last_half=half))
    torch.cuda.synchronize()
    assert_same_league(kit, lg, m, ref, sd, games, block)
    T = int(m["lengths"].max())
    assert T == max(int(r["lengths"].max()) for r in ref["per"]) and lg.step_counter == c0 + T
    assert int(half) == LIMIT & 1
    assert [int(k._ctr[0]) for k in kit["kernels"]] == ctrs == [7, 11, 15]
    if games == 37:  # equality must not pass on matches that all look alike
        w = lg.winner_id.view(len(PAIRS), block)[:6, :games]
        hits = int((w != 0).sum())
        distinct = {tuple(r["lengths"].tolist()) for r in ref["per"][:6]}
        print(f"{reward}: {hits} hits over the six pairings, {len(distinct)} distinct lengths vectors, "
              f"shortest {min(int(r['lengths'].min()) for r in ref['per'][:6])}")
        assert hits >= 8 and len(distinct) >= 5


def test_act_league_in_chunks(kit, monkeypatch):
    """launches of 7 ticks, each continuing the last (resume=True), until no
    game plays any more: one launch's lengths, returns and final states"""
    monkeypatch.setenv("SK_FWD16", "0")
    games, block = 37, 64
    ref = match_reference(kit, games, "looking")
    lg, sd, obs = league_env(kit, ref, games, block)
    c0 = lg.step_counter
    m = lg.act_league(kit["kernels"], PAIRS, block, obs, n_ticks=7)
    launches = 1
    while int(m["call_lengths"].max()) > 0:
        m = lg.act_league(kit["kernels"], PAIRS, block, m["obs"], n_ticks=7, out=m, resume=True)
        launches += 1
        assert launches < 20
    torch.cuda.synchronize()
    T = max(int(r["lengths"].max()) for r in ref["per"])
    assert launches == -(-T // 7) + 1  # the last launch finds every game ended
    assert_same_league(kit, lg, m, ref, sd, games, block)
    assert lg.step_counter == c0 + T


def test_act_league_under_capture(kit, monkeypatch):
    """one act_league captured on a side stream with the buffers and device
    tables of an eager call (nothing is allocated or uploaded) and replayed
    once from the reloaded start: the eager result"""
    monkeypatch.setenv("SK_FWD16", "0")
    games, block = 37, 64
    ref = match_reference(kit, games, "looking")
    lg, sd, obs = league_env(kit, ref, games, block)
    bufs = lg.act_league(kit["kernels"], PAIRS, block, obs, n_ticks=LIMIT)  # eager: buffers, tables, warm launch
    torch.cuda.synchronize()
    assert_same_league(kit, lg, bufs, ref, sd, games, block)
    lg.load_state_dict(sd)
    obs0 = obs.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        lg.sync_step_counter()
        with torch.cuda.graph(graph, stream=side):
            m = lg.act_league(kit["kernels"], PAIRS, block, obs0, n_ticks=LIMIT, out=bufs)
    torch.cuda.synchronize()
    assert m["nets"] is bufs["nets"] and m["pairs"] is bufs["pairs"]
    for t in (m["lengths"], m["returns"], m["obs"]):
        t.zero_()
    lg.load_state_dict(sd)
    with torch.cuda.stream(side):
        lg.sync_step_counter()
        graph.replay()
    torch.cuda.synchronize()
    assert_same_league(kit, lg, m, ref, sd, games, block)


def test_act_league_skips_a_pairing_outside_the_table(kit, monkeypatch):
    """a pair index equal to K, written straight into the device table (the
    host check never sees it): the kernel's guard leaves that block's games
    alone — lengths 0, returns 0, planes as loaded — and the other pairings
    play as before"""
    monkeypatch.setenv("SK_FWD16", "0")
    games, block, bad = 37, 64, 3
    ref = match_reference(kit, games, "looking")
    lg, sd, obs = league_env(kit, ref, games, block)
    with pytest.raises(ValueError):  # the host check
        lg.act_league(kit["kernels"], PAIRS[:bad] + [(1, 3)] + PAIRS[bad + 1:], block, obs, n_ticks=LIMIT)
    m = lg.act_league(kit["kernels"], PAIRS, block, obs, n_ticks=LIMIT)
    torch.cuda.synchronize()
    lg.load_state_dict(sd)
    m["pairs"][bad, 1] = len(kit["kernels"])
    m["call_lengths"].fill_(-1)
    m = lg.act_league(kit["kernels"], PAIRS, block, obs, n_ticks=LIMIT, out=m)  # same host pairs: no upload
    torch.cuda.synchronize()
    assert m["pairs"][bad].tolist() == [PAIRS[bad][0], len(kit["kernels"])]
    assert_same_league(kit, lg, m, ref, sd, games, block, skip=(bad,))
    P = len(PAIRS)
    assert int(m["lengths"].view(P, block)[bad].abs().sum()) == 0
    assert int((m["returns"].view(2, P, block)[:, bad] != 0).sum()) == 0
    for name, _, w in kit["PLANES"]:
        got = getattr(lg, name).view(P, block, w)[bad]
        want = torch.as_tensor(sd[name]).view(P, block, w)[bad].cuda()
        assert torch.equal(bits(got), bits(want)), name


def gpu_learner(kit, seed=9, n_envs=64, tick_limit=40):
    torch.manual_seed(seed)
    return kit["learner"].SkillshotLearner(n_envs=n_envs, device="cuda", seed=seed, tick_limit=tick_limit,
                                           precision="fp32")


def test_league_kernel_equals_pairwise(kit, monkeypatch):
    """league's one launch and its pair-by-pair path (SK_LEAGUE_KERNEL=0)
    return the same dict, and its entries are pairwise evaluate's legs.  100
    games: blocks of 128, four workgroups per pairing, 28 pad games."""
    monkeypatch.setenv("SK_FWD16", "0")
    L = gpu_learner(kit)
    with torch.no_grad():
        L.model_actor.load_state_dict(kit["nets"][0].state_dict())
    actors = [None, kit["nets"][1], kit["nets"][2]]
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("SK_LEAGUE_KERNEL", flag)
        res[flag] = L.league(actors, games=100, tick_limit=LIMIT, seed=ENV_SEED)
    print(res["1"])
    assert res["1"] == res["0"]
    assert len(L._league_envs) == 1 and next(iter(L._league_envs.values())).n == 6 * 128
    monkeypatch.setenv("SK_LEAGUE_KERNEL", "1")
    assert L.league(actors, games=100, tick_limit=LIMIT, seed=ENV_SEED) == res["1"]  # the cached env, rewound
    r = res["1"]
    hits = 0
    for j in (1, 2):
        e = L.evaluate(opponent=kit["nets"][j], games=100, tick_limit=LIMIT, seed=ENV_SEED)
        leg1, leg2 = e["legs"]
        assert (r["seat_wins"][0][j], r["seat_losses"][0][j], r["seat_draws"][0][j]) == \
            (leg1["wins"], leg1["losses"], leg1["draws"])
        assert (r["seat_wins"][j][0], r["seat_losses"][j][0], r["seat_draws"][j][0]) == \
            (leg2["losses"], leg2["wins"], leg2["draws"])
        assert r["mean_ticks"][0][j] == leg1["mean_ticks"] and r["mean_ticks"][j][0] == leg2["mean_ticks"]
        for got, want in ((r["mean_return"][0][j], leg1["mean_return"]),
                          (r["opponent_mean_return"][0][j], leg1["opponent_mean_return"]),
                          (r["mean_return"][j][0], leg2["opponent_mean_return"]),
                          (r["opponent_mean_return"][j][0], leg2["mean_return"])):
            assert abs(got - want) <= 1e-9 * max(abs(got), abs(want))
        assert r["wins"][0][j] == e["wins"] and r["wins"][j][0] == e["losses"] and r["draws"][0][j] == e["draws"]
        hits += e["wins"] + e["losses"]
    assert hits >= 6
    assert sorted(r["ranking"]) == [0, 1, 2]


def test_league_leaves_training_untouched(kit, monkeypatch):
    """two learners with one seed train an epoch, one of them plays a league,
    both train another: the same nets bit for bit, the same step counters and
    noise call numbers"""
    monkeypatch.setenv("SK_FWD16", "0")
    out = []
    for plays in (False, True):
        L = gpu_learner(kit)
        L.model_train(1)
        if plays:
            a = L.league([None, kit["nets"][1], kit["nets"][2]], games=96, tick_limit=40)
            assert a["n_actors"] == 3 and a["games"] == 96
        L.model_train(1)
        torch.cuda.synchronize()
        out.append(([p.detach().clone() for m in (L.model_actor, L.model_critic) for p in m.parameters()],
                    L.game_environment.step_counter, L.actor_kernel.calls,
                    torch.stack(L.progress["epoch_ticks"])))
    (pa, sa, ca, ta), (pb, sb, cb, tb) = out
    for x, y in zip(pa, pb):
        assert torch.equal(x, y)
    assert sa == sb and ca == cb and torch.equal(ta, tb)
