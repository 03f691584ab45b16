"""Opponent-pool training on the GPU: one sk_env_act_step_pool launch per tick
(k_act_step_pool32: each block of 32 games acting from the two actors its
pairing names, the learner with its exploration noise, then the step and the
ring insert) against the launches it replaces, bit for bit: every seated
actor's forward on the whole observation, a select by (seat, block), and
step_insert / step.  Also: all-(0, 0) pairs against the self-play act_step,
graph capture, the guard on a pair index outside the table, and
SkillshotLearner.train_vs's two paths and what it must leave alone."""
import pytest
import torch

pytestmark = pytest.mark.gpu

LIMIT, TICKS = 25, 40
ENV_SEED = 6
ACTOR_SEEDS = (41, 42, 43)  # test_pool_cpu's: they turn, move and hit inside 25 ticks
CTR0 = (7, 11, 15)          # noise call numbers with a history
# (N, block, pairs): two blocks, one per seating; a self-play block, a mixed one and one without the learner;
# two workgroups per pairing
SHAPES = {64: (32, [(0, 1), (1, 0)]), 96: (32, [(0, 0), (0, 1), (2, 1)]), 128: (64, [(0, 2), (1, 0)])}
MODES = {"param": (0.5, 0.0), "action": (0.0, 0.15), "none": (0.0, 0.0)}
OUT_KEYS = ("actions", "obs", "reward", "done", "winner", "obs_reset")


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
    return dict(ssa=ssa, learner=learner, nets=nets, kernels=kernels, PLANES=PLANES, turning_actor=turning_actor)


def bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype != torch.bool else t


def set_counters(kit):
    for k, c in zip(kit["kernels"], CTR0):
        k._ctr.zero_()
        k._ctr[0] = c


def fresh_env(kit, n):
    g = kit["ssa"].VecSkillshotGame(n, device="cuda", seed=ENV_SEED, tick_limit=LIMIT)
    g.step_counter = 0
    g.reset(random_positions=True)
    return g


def fresh_ring(kit, n, with_ring):
    # 7 ticks and 5 rows: no multiple of 2N, so the 40 ticks wrap it five times, each time inside a tick
    return kit["learner"].ReplayRing(7 * 2 * n + 5, "cuda") if with_ring else None


def composed_tick(kit, g, pairs, block, obs, noisy, sds, ring, reward):
    """the launches the pool tick replaces: every seated actor's forward on the
    [2N] rows, each (seat, block) taking its actor's rows, then step_insert / step"""
    x = obs.reshape(-1, 12)
    seat = torch.tensor(pairs, device="cuda").t().repeat_interleave(block, dim=1)  # [2, N]
    act = torch.zeros((2, g.n, 2), device="cuda")
    for k in sorted({i for pr in pairs for i in pr}):
        sd, asd = sds if k == noisy else (0.0, 0.0)
        a = kit["kernels"][k](x, noise_sd=sd, action_sd=asd).view(2, g.n, 2)
        act = torch.where((seat == k)[:, :, None], a, act)
    act = act.contiguous()
    if ring is not None:
        out = g.step_insert(act, obs, ring, reward=reward, auto_reset=True, reset_obs=True)
    else:
        out = g.step(act, obs=True, reward=reward, auto_reset=True, reset_obs=True)
    out["actions"] = act
    return out


def run(kit, n, block, pairs, sds, reward, with_ring, tick, ticks=TICKS):
    """`ticks` ticks from the fresh start: per-tick outputs, final planes, ring, counters"""
    set_counters(kit)
    g = fresh_env(kit, n)
    ring = fresh_ring(kit, n, with_ring)
    obs = g.observe()[0].clone()
    step0 = g.step_counter
    per = []
    for _ in range(ticks):
        out = tick(g, obs, ring)
        per.append({k: out[k].clone() for k in OUT_KEYS})
        obs = per[-1]["obs_reset"]
    torch.cuda.synchronize()
    return dict(per=per, planes={name: getattr(g, name).clone() for name, _, _ in kit["PLANES"]},
                ring=None if ring is None else (ring.buf.clone(), int(ring.total_t), ring.total),
                step=g.step_counter, stepped=g.step_counter - step0, calls=[k.calls for k in kit["kernels"]], counters=g.counters())


def assert_same_run(a, b):
    for t, (x, y) in enumerate(zip(a["per"], b["per"])):
        for k in OUT_KEYS:
            assert torch.equal(bits(x[k]), bits(y[k])), (t, k)
    for name in a["planes"]:
        assert torch.equal(bits(a["planes"][name]), bits(b["planes"][name])), name
    assert (a["ring"] is None) == (b["ring"] is None)
    if a["ring"] is not None:
        assert a["ring"][1:] == b["ring"][1:]
        assert torch.equal(bits(a["ring"][0]), bits(b["ring"][0]))
    assert a["step"] == b["step"] and a["calls"] == b["calls"] and a["counters"] == b["counters"]


@pytest.mark.parametrize("with_ring", [True, False], ids=["ring", "noring"])
@pytest.mark.parametrize("reward", ["looking", "simple"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n", list(SHAPES))
def test_pool_tick_equals_the_composition(kit, monkeypatch, n, mode, reward, with_ring):
    monkeypatch.setenv("SK_FWD16", "0")
    block, pairs = SHAPES[n]
    sds = MODES[mode]

    def pool(g, obs, ring):
        return g.act_step_pool(kit["kernels"], pairs, block, obs, noisy=0, noise_sd=sds[0], action_sd=sds[1],
                               ring=ring, reward=reward)

    got = run(kit, n, block, pairs, sds, reward, with_ring, pool)
    want = run(kit, n, block, pairs, sds, reward, with_ring,
               lambda g, obs, ring: composed_tick(kit, g, pairs, block, obs, 0, sds, ring, reward))
    assert_same_run(got, want)
    assert got["stepped"] == TICKS
    # the noisy actor drew once per tick, nobody else's call number moved
    assert got["calls"] == [CTR0[0] + (TICKS if mode != "none" else 0), CTR0[1], CTR0[2]]
    if with_ring:
        assert got["ring"][1] == got["ring"][2] == TICKS * 2 * n > 5 * (7 * 2 * n + 5)
    c = got["counters"]
    hits, limit = c["hits_p1"] + c["hits_p2"], c["dones"] - c["hits_p1"] - c["hits_p2"]
    print(f"N={n} {mode} {reward} ring={with_ring}: {hits} ends by a hit, {limit} at the tick limit")
    # games end both ways and restart inside the run (every game not hit ends at tick 25 and plays on)
    assert hits >= 1 and limit >= n // 2
    if mode != "none":  # the learner's rows carry noise, the opponents' do not
        seat = torch.tensor(pairs, device="cuda").t().repeat_interleave(block, dim=1)
        x = got["per"][0]
        obs0 = fresh_env(kit, n).observe()[0]
        for k in range(3):
            clean = kit["kernels"][k](obs0.reshape(-1, 12)).view(2, n, 2)
            same = (x["actions"] == clean).all(-1)[seat == k]
            assert bool(same.all()) if k != 0 else not bool(same.any()), k


def test_all_self_play_pairs_equal_act_step(kit, monkeypatch):
    """every block (0, 0): the parent's self-play tick on a twin env"""
    monkeypatch.setenv("SK_FWD16", "0")
    n, sds = 64, MODES["param"]
    got = run(kit, n, 32, [(0, 0), (0, 0)], sds, "looking", True,
              lambda g, obs, ring: g.act_step_pool(kit["kernels"], [(0, 0), (0, 0)], 32, obs, noisy=0,
                                                   noise_sd=sds[0], action_sd=sds[1], ring=ring))
    want = run(kit, n, 32, None, sds, "looking", True,
               lambda g, obs, ring: g.act_step(kit["kernels"][0], obs, noise_sd=sds[0], action_sd=sds[1], ring=ring))
    assert_same_run(got, want)
    assert got["calls"][0] == CTR0[0] + TICKS and got["counters"]["dones"] >= n


def test_two_pool_ticks_under_capture(kit, monkeypatch):
    """two ticks (obs ping-pong) captured as one graph with the buffers and
    tables of an eager call, replayed 10 times: 20 eager ticks"""
    monkeypatch.setenv("SK_FWD16", "0")
    n, sds = 96, MODES["param"]
    block, pairs = SHAPES[n]

    def pool(g, obs, ring, out=None):
        return g.act_step_pool(kit["kernels"], pairs, block, obs, noisy=0, noise_sd=sds[0], action_sd=sds[1],
                               ring=ring, out=out)

    want = run(kit, n, block, pairs, sds, "looking", True, pool, ticks=20)
    set_counters(kit)
    g = fresh_env(kit, n)
    start = g.state_dict()
    ring = fresh_ring(kit, n, True)
    obs_a = g.observe()[0].clone()
    obs0 = obs_a.clone()
    b1 = pool(g, obs_a, ring)                  # eager: buffers, tables, warm launches
    obs_b = b1["obs_reset"]
    b2 = pool(g, obs_b, ring)
    b2 = pool(g, obs_b, ring, out=dict(b2, obs_reset=obs_a))  # tick 2 writes the observation tick 1 reads
    torch.cuda.synchronize()
    g.load_state_dict(start)
    set_counters(kit)
    ring.buf.zero_()
    ring.total_t.zero_()
    g.clear_counters()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        g.sync_step_counter()
        with torch.cuda.graph(graph, stream=side):
            m1 = pool(g, obs_a, ring, out=b1)
            m2 = pool(g, obs_b, ring, out=b2)
    torch.cuda.synchronize()
    assert m1["nets"] is b1["nets"] and m1["pairs"] is b1["pairs"] and m2["obs_reset"] is obs_a
    g.load_state_dict(start)
    set_counters(kit)
    ring.buf.zero_()
    ring.total_t.zero_()
    g.clear_counters()
    obs_a.copy_(obs0)
    with torch.cuda.stream(side):
        g.sync_step_counter()
        for _ in range(10):
            graph.replay()
    torch.cuda.synchronize()
    for k in OUT_KEYS:  # the last two ticks' outputs
        assert torch.equal(bits(m1[k]), bits(want["per"][18][k])), k
        assert torch.equal(bits(m2[k]), bits(want["per"][19][k])), k
    for name, _, _ in kit["PLANES"]:
        assert torch.equal(bits(getattr(g, name)), bits(want["planes"][name])), name
    assert torch.equal(bits(ring.buf), bits(want["ring"][0])) and int(ring.total_t) == want["ring"][1] == 20 * 2 * n
    assert g.step_counter == want["step"] and want["stepped"] == 20
    assert [k.calls for k in kit["kernels"]] == want["calls"] == [CTR0[0] + 20, CTR0[1], CTR0[2]]
    assert g.counters() == want["counters"]


def test_pool_tick_skips_a_pairing_outside_the_table(kit, monkeypatch):
    """a pair index equal to K, written straight into the device table (the
    host check never sees it): that block's planes, outputs, actions and ring
    rows stay as they were, the other blocks tick as before, and the ring's
    total, the step counter and the call number still advance"""
    monkeypatch.setenv("SK_FWD16", "0")
    n, sds, bad = 96, MODES["param"], 1
    block, pairs = SHAPES[n]
    K = len(kit["kernels"])
    want = run(kit, n, block, pairs, sds, "looking", True,
               lambda g, obs, ring: g.act_step_pool(kit["kernels"], pairs, block, obs, noisy=0, noise_sd=sds[0],
                                                    action_sd=sds[1], ring=ring), ticks=1)
    set_counters(kit)
    g = fresh_env(kit, n)
    ring = fresh_ring(kit, n, True)
    obs = g.observe()[0].clone()
    with pytest.raises(ValueError):  # the host check
        g.act_step_pool(kit["kernels"], pairs[:bad] + [(0, K)] + pairs[bad + 1:], block, obs, noisy=0)
    start = g.state_dict()
    m = g.act_step_pool(kit["kernels"], pairs, block, obs, noisy=0, noise_sd=sds[0], action_sd=sds[1], ring=ring)
    torch.cuda.synchronize()
    g.load_state_dict(start)
    set_counters(kit)
    g.clear_counters()
    ring.total_t.zero_()
    ring.total = 0
    ring.buf.fill_(-3.0)
    for k in OUT_KEYS:
        m[k].fill_(77)
    m["pairs"][bad, 1] = K
    m = g.act_step_pool(kit["kernels"], pairs, block, obs, noisy=0, noise_sd=sds[0], action_sd=sds[1], ring=ring,
                        out=m, actions=m["actions"])  # same host pairs: no upload
    torch.cuda.synchronize()
    assert m["pairs"][bad].tolist() == [pairs[bad][0], K]
    blk = slice(bad * block, (bad + 1) * block)
    keep = torch.ones(n, dtype=torch.bool, device="cuda")
    keep[blk] = False
    w = want["per"][0]
    for k in OUT_KEYS:
        games = m[k] if m[k].dim() == 1 else m[k].transpose(0, 1)      # game-major
        ref = w[k] if w[k].dim() == 1 else w[k].transpose(0, 1)
        assert torch.equal(bits(games[keep]), bits(ref[keep])), k
        assert bool((games[blk] == 77).all()), k
    for name, _, wd in kit["PLANES"]:
        got = getattr(g, name).view(n, wd)
        assert torch.equal(bits(got[keep]), bits(want["planes"][name].view(n, wd)[keep])), name
        assert torch.equal(bits(got[blk]), bits(torch.as_tensor(start[name]).view(n, wd)[blk].cuda())), name
    rows = ring.buf[:2 * n].view(2, n, 28)
    assert torch.equal(bits(rows[:, keep]), bits(want["ring"][0][:2 * n].view(2, n, 28)[:, keep]))
    assert bool((rows[:, blk] == -3.0).all()) and bool((ring.buf[2 * n:] == -3.0).all())
    assert int(ring.total_t) == 2 * n and g.step_counter == start["step_counter"] + 1
    assert [k.calls for k in kit["kernels"]] == [CTR0[0] + 1, CTR0[1], CTR0[2]]


def gpu_learner(kit, seed=5, n_envs=128, exploration="param_noise"):
    torch.manual_seed(seed)
    L = kit["learner"].SkillshotLearner(n_envs=n_envs, device="cuda", seed=seed, tick_limit=LIMIT, precision="fp32",
                                        replay_capacity=4096, exploration=exploration)
    with torch.no_grad():
        L.model_actor.load_state_dict(kit["nets"][0].state_dict())
    return L


@pytest.mark.parametrize("exploration", ["param_noise", "action_noise"])
def test_train_vs_kernel_equals_the_loop_path(kit, monkeypatch, exploration):
    """no updates (warmup beyond reach): one launch per tick and SK_POOL_KERNEL=0
    leave the same env planes, ring, step counter and call number; the ring
    (4,096 rows) wraps inside the 30 ticks of 320 rows"""
    monkeypatch.setenv("SK_FWD16", "0")
    opp = [kit["nets"][1], kit["nets"][2]]
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("SK_POOL_KERNEL", flag)
        L = gpu_learner(kit, n_envs=160, exploration=exploration)  # five blocks: the two opponents' four and a (0, 0)
        c0 = L.game_environment.step_counter
        assert L.train_vs(opp, 30, warmup=1 << 30, self_play=1) == []
        torch.cuda.synchronize()
        g = L.game_environment
        res[flag] = ({name: getattr(g, name).clone() for name, _, _ in kit["PLANES"]}, L.replay.buf.clone(),
                     int(L.replay.total_t), L.replay.total, g.step_counter - c0, L.actor_kernel.calls, g.counters())
    a, b = res["1"], res["0"]
    for name in a[0]:
        assert torch.equal(bits(a[0][name]), bits(b[0][name])), name
    assert torch.equal(bits(a[1]), bits(b[1]))
    assert a[2:] == b[2:] and a[2] == a[3] == 30 * 320 and a[4] == 30 and a[5] == 30
    assert a[6]["dones"] >= 160


def test_train_vs_trains_and_leaves_the_rest_alone(kit, monkeypatch):
    """with updates the actor changes and the opponents' nets do not; evaluate
    afterwards returns what a learner that never trained against a pool
    returns for the same nets; and train_ticks carries on from train_vs's env
    and ring: the one-launch path and SK_POOL_KERNEL=0, each followed by
    train_ticks and a second train_vs, end with the same nets bit for bit"""
    monkeypatch.setenv("SK_FWD16", "0")
    opp = [kit["turning_actor"](s).cuda() for s in ACTOR_SEEDS[1:]]
    before = [{k: v.clone() for k, v in o.state_dict().items()} for o in opp]
    out = []
    for flag in ("1", "0"):
        monkeypatch.setenv("SK_POOL_KERNEL", flag)
        L = gpu_learner(kit)
        mine = [p.detach().clone() for p in L.model_actor.parameters()]
        s0 = L.game_environment.step_counter
        stats = L.train_vs(opp, 6, batch=64, warmup=0)
        assert len(stats) == 6 and L.replay.total == 6 * 256 == int(L.replay.total_t)
        assert any(not torch.equal(p, q) for p, q in zip(L.model_actor.parameters(), mine))
        for o, b in zip(opp, before):
            assert all(torch.equal(v, b[k]) for k, v in o.state_dict().items())
        if flag == "1":
            fresh = gpu_learner(kit)  # never trained against a pool; the same actor
            with torch.no_grad():
                fresh.model_actor.load_state_dict(L.model_actor.state_dict())
            assert L.evaluate(opponent=opp[0], games=64, tick_limit=LIMIT) == \
                fresh.evaluate(opponent=opp[0], games=64, tick_limit=LIMIT)
        c0, k0 = L.game_environment.step_counter, L.actor_kernel.calls
        assert c0 == s0 + 6 and k0 == 6
        assert len(L.train_ticks(3, batch=64, warmup=0)) == 3
        assert len(L.train_vs(opp, 2, batch=64, warmup=0)) == 2
        torch.cuda.synchronize()
        assert L.game_environment.step_counter == c0 + 5 and L.actor_kernel.calls == k0 + 5
        assert L.replay.total == 11 * 256 == int(L.replay.total_t)
        out.append([p.detach().clone() for m in (L.model_actor, L.model_critic) for p in m.parameters()])
    for x, y in zip(*out):
        assert torch.equal(x, y)
