"""Head-to-head matches on the GPU: one sk_env_act_match launch (two actors,
one per seat, whole matches) against the per-tick loop built from the
launches it replaces — sk_actor_forward_f32 per seat (32-row tiles,
SK_FWD16=0: the match kernel's tile) and sk_env_step — bit for bit; the match
played in chunks and under graph capture; SkillshotLearner.evaluate's two
paths; and evaluate's promise to leave training alone."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

LIMIT = 60
ENV_SEED = 6
ACTOR_SEEDS = (23, 24)  # chosen on the CPU loop path: 228 games give >= 8 hits per seat, > 200 draws, short games


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
        kern._ctr[0] = 7 + 4 * k  # noise call numbers with a history: a match must not move them
    return dict(ssa=ssa, learner=learner, nets=nets, kernels=kernels, PLANES=PLANES)


def fresh_env(kit, n, config=None):
    """config: a name of tests/config_cases.py's table (None: the reference's constants)"""
    cfg = None
    if config is not None:
        import config_cases
        cfg = config_cases.sk_config(config)
    g = kit["ssa"].VecSkillshotGame(n, device="cuda", seed=ENV_SEED, tick_limit=LIMIT, config=cfg)
    g.step_counter = 0
    g.reset(random_positions=True)
    return g


_LOOPS = {}


def loop_reference(kit, n, reward, swapped, config=None):
    """the per-tick loop, once per case (shared, never modified): lengths, the
    loop's fp32 acc += r over live games, every plane and the obs of each
    game at the moment it ended (the loop keeps moving ended games' players;
    the snapshots stop with the game), and the loop's iterations"""
    key = (n, reward, swapped, config)
    if key in _LOOPS:
        return _LOOPS[key]
    k1, k2 = kit["kernels"][::-1] if swapped else kit["kernels"]
    g = fresh_env(kit, n, config)
    start = g.state_dict()
    obs, _ = g.observe()
    obs0 = obs.clone()
    alive = torch.ones(n, dtype=torch.bool, device="cuda")
    acc = torch.zeros((2, n), device="cuda")
    lengths = torch.zeros(n, dtype=torch.int32, device="cuda")
    planes = {name: getattr(g, name).clone() for name, _, _ in kit["PLANES"]}
    final_obs = obs.clone()
    iters = 0
    while bool(alive.any()):
        act = torch.stack((k1(obs[0]), k2(obs[1])))
        out = g.step(act, obs=True, reward=reward, auto_reset=False)
        acc = torch.where(alive[None], acc + out["reward"], acc)
        lengths += alive.int()
        for name in planes:
            planes[name] = torch.where(alive[:, None], getattr(g, name), planes[name])
        final_obs = torch.where(alive[None, :, None], out["obs"], final_obs)
        alive = alive & ~out["done"].bool()
        obs = out["obs"]
        iters += 1
    torch.cuda.synchronize()
    _LOOPS[key] = dict(start=start, obs0=obs0, lengths=lengths, returns=acc, planes=planes, obs=final_obs,
                       iters=iters, step_counter=g.step_counter)
    return _LOOPS[key]


def bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype != torch.bool else t


def assert_same_match(kit, g, m, ref):
    assert torch.equal(m["lengths"], ref["lengths"])
    assert torch.equal(bits(m["returns"]), bits(ref["returns"]))
    for name, _, _ in kit["PLANES"]:
        assert torch.equal(bits(getattr(g, name)), bits(ref["planes"][name])), name
    assert torch.equal(bits(m["obs"]), bits(ref["obs"]))


@pytest.mark.parametrize("swapped", [False, True], ids=["AB", "BA"])
@pytest.mark.parametrize("reward", ["looking", "simple"])
@pytest.mark.parametrize("n", [228, 37, 32, 1])
def test_act_match_equals_per_tick_loop(kit, monkeypatch, n, reward, swapped):
    """228 games: 7 workgroups and a tail of 4 games; 37: odd N, a tail of 5;
    32: exactly one workgroup; 1: a single game.  Both seatings: each seat
    must read its own net."""
    monkeypatch.setenv("SK_FWD16", "0")
    ref = loop_reference(kit, n, reward, swapped)
    k1, k2 = kit["kernels"][::-1] if swapped else kit["kernels"]
    ctrs = [int(k._ctr[0]) for k in kit["kernels"]]
    g = fresh_env(kit, n)
    g.load_state_dict(ref["start"])
    c0 = g.step_counter
    half = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    m = g.act_match(k1, k2, ref["obs0"], n_ticks=LIMIT + 20, reward=reward, out=dict(last_half=half))
    torch.cuda.synchronize()
    assert_same_match(kit, g, m, ref)
    T = int(m["lengths"].max())
    assert T == ref["iters"] and g.step_counter == c0 + T == ref["step_counter"]
    assert int(half) == (LIMIT + 20) & 1
    assert [int(k._ctr[0]) for k in kit["kernels"]] == ctrs == [7, 11]
    if n == 228:
        w, ln = g.winner_id, m["lengths"]
        hit1, hit2, draws = int((w == 1).sum()), int((w == 2).sum()), int((w == 0).sum())
        print(f"n={n} {reward} swapped={swapped}: hit on seat 1 / seat 2 / draws {hit1}/{hit2}/{draws}, "
              f"shortest {int(ln.min())}")
        assert hit1 >= 3 and hit2 >= 3 and draws >= 3 and int(ln.min()) < 10
        assert torch.equal(ln[w == 0], torch.full_like(ln[w == 0], LIMIT))
        other = loop_reference(kit, n, reward, not swapped)  # the seats swapped: another match
        assert not torch.equal(m["lengths"], other["lengths"])
        assert not torch.equal(bits(m["returns"]), bits(other["returns"]))


def test_act_match_equals_per_tick_loop_at_cfg_packed(kit, monkeypatch):
    """the match kernel instantiates the step on its own: one case (37 games) at a configuration in which
    every constant differs from the reference's (tests/config_cases.py: cfg_packed)"""
    monkeypatch.setenv("SK_FWD16", "0")
    n, reward = 37, "looking"
    ref = loop_reference(kit, n, reward, False, config="cfg_packed")
    k1, k2 = kit["kernels"]
    g = fresh_env(kit, n, "cfg_packed")
    g.load_state_dict(ref["start"])
    c0 = g.step_counter
    m = g.act_match(k1, k2, ref["obs0"], n_ticks=LIMIT + 20, reward=reward)
    torch.cuda.synchronize()
    assert_same_match(kit, g, m, ref)
    T = int(m["lengths"].max())
    assert T == ref["iters"] and g.step_counter == c0 + T == ref["step_counter"]
    # (and it is another match than the reference configuration's)
    assert not torch.equal(m["lengths"], loop_reference(kit, n, reward, False)["lengths"]) or \
        not torch.equal(bits(m["returns"]), bits(loop_reference(kit, n, reward, False)["returns"]))


def test_act_match_in_chunks(kit, monkeypatch):
    """launches of 7 ticks, each continuing the last, until no game plays any
    more: the totals, the final states and the returns (summed in tick order
    across the launches) equal the single launch's"""
    monkeypatch.setenv("SK_FWD16", "0")
    n = 100
    ref = loop_reference(kit, n, "looking", False)
    k1, k2 = kit["kernels"]
    g = fresh_env(kit, n)
    g.load_state_dict(ref["start"])
    c0 = g.step_counter
    m = g.act_match(k1, k2, ref["obs0"], n_ticks=7)
    launches = 1
    while int(m["call_lengths"].max()) > 0:
        m = g.act_match(k1, k2, m["obs"], n_ticks=7, out=m, resume=True)
        launches += 1
        assert launches < 20
    torch.cuda.synchronize()
    assert launches == -(-ref["iters"] // 7) + 1  # the last launch finds every game ended
    assert_same_match(kit, g, m, ref)
    assert g.step_counter == c0 + ref["iters"]
    single = fresh_env(kit, n)
    single.load_state_dict(ref["start"])
    s = single.act_match(k1, k2, ref["obs0"], n_ticks=LIMIT)
    for key in ("lengths", "returns", "obs"):
        assert torch.equal(bits(s[key]), bits(m[key])), key


def test_act_match_under_capture(kit, monkeypatch):
    """one act_match captured on a side stream (a linear chain: a copy, a
    memset, the match launch, the counter launch, the obs select) and
    replayed once from the reloaded start: the eager result"""
    monkeypatch.setenv("SK_FWD16", "0")
    n = 37
    ref = loop_reference(kit, n, "looking", False)
    k1, k2 = kit["kernels"]
    g = fresh_env(kit, n)
    g.load_state_dict(ref["start"])
    bufs = g.act_match(k1, k2, ref["obs0"], n_ticks=LIMIT)  # eager: allocates the buffers, warms the launch
    torch.cuda.synchronize()
    assert_same_match(kit, g, bufs, ref)
    g.load_state_dict(ref["start"])
    obs0 = ref["obs0"].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        g.sync_step_counter()
        with torch.cuda.graph(graph, stream=side):
            m = g.act_match(k1, k2, obs0, n_ticks=LIMIT, out=bufs)
    torch.cuda.synchronize()
    for t in (m["lengths"], m["returns"], m["obs"]):
        t.zero_()
    g.load_state_dict(ref["start"])
    with torch.cuda.stream(side):
        g.sync_step_counter()
        graph.replay()
    torch.cuda.synchronize()
    assert_same_match(kit, g, m, ref)


def gpu_learner(kit, seed=9, n_envs=64, tick_limit=40):
    torch.manual_seed(seed)
    return kit["learner"].SkillshotLearner(n_envs=n_envs, device="cuda", seed=seed, tick_limit=tick_limit,
                                           precision="fp32")


def test_evaluate_kernel_equals_loop(kit, monkeypatch):
    """evaluate's one-launch legs and its per-tick loop (SK_MATCH_KERNEL=0):
    the same integer tallies and mean_ticks, and the mean returns equal as
    fp32 sums (the whole dicts are equal)"""
    monkeypatch.setenv("SK_FWD16", "0")
    L = gpu_learner(kit)
    with torch.no_grad():
        L.model_actor.load_state_dict(kit["nets"][0].state_dict())
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("SK_MATCH_KERNEL", flag)
        res[flag] = L.evaluate(opponent=kit["nets"][1], games=228, tick_limit=LIMIT, seed=ENV_SEED)
    print(res["1"])
    assert res["1"] == res["0"]
    r = res["1"]
    assert r["games"] == 456 and r["wins"] + r["losses"] + r["draws"] == 456
    assert r["wins"] >= 6 and r["losses"] >= 6 and r["draws"] >= 6
    # leg 1 is the (A, B) match of the loop reference: seat 1's wins are the hits on seat 2
    ref = loop_reference(kit, 228, "looking", False)
    w = (ref["planes"]["misc"][:, 1] >> 24) & 0xFF
    assert r["legs"][0]["wins"] == int((w == 2).sum()) and r["legs"][0]["losses"] == int((w == 1).sum())
    assert r["legs"][0]["mean_return"] == float(ref["returns"][0].sum().double()) / 228
    mirror = L.evaluate(opponent=None, games=228, tick_limit=LIMIT)
    assert mirror["wins"] == mirror["losses"] and mirror["legs"][0]["wins"] == mirror["legs"][1]["losses"]


def test_evaluate_leaves_training_untouched(kit, monkeypatch):
    """two learners with one seed train an epoch, one of them evaluates
    (against a module and against itself), both train another: the same nets
    bit for bit, the same step counters and noise call numbers"""
    monkeypatch.setenv("SK_FWD16", "0")
    out = []
    for evaluates in (False, True):
        L = gpu_learner(kit)
        L.model_train(1)
        if evaluates:
            a = L.evaluate(opponent=kit["nets"][1], games=96, tick_limit=40)
            b = L.evaluate(opponent=None, games=96, tick_limit=40)
            assert a["games"] == b["games"] == 192
        L.model_train(1)
        torch.cuda.synchronize()
        out.append(([p.detach().clone() for m in (L.model_actor, L.model_critic) for p in m.parameters()],
                    L.game_environment.step_counter, L.actor_kernel.calls,
                    torch.stack(L.progress["epoch_ticks"])))
    (pa, sa, ca, ta), (pb, sb, cb, tb) = out
    for x, y in zip(pa, pb):
        assert torch.equal(x, y)
    assert sa == sb and ca == cb and torch.equal(ta, tb)
