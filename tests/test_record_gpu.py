"""Match records on the GPU: the recording launches (sk_env_act_match_rec /
sk_env_act_league_rec) against a per-tick loop that snapshots every game's
planes, actions and rewards each tick, bit for bit, with the record filled
with a byte pattern first so that every byte a launch must not write shows;
the match's own outputs against test_match_gpu's loop reference; a record made
in chunks and under graph capture; the league's rows against two-actor match
records; SkillshotLearner.evaluate / league on the kernel path against the
loop path; and the record's boards against the CPU painter."""
import pytest
import torch

from test_match_gpu import ENV_SEED, LIMIT, assert_same_match, fresh_env, kit, loop_reference  # noqa: F401
import test_league_gpu as lgt

pytestmark = pytest.mark.gpu

PATTERN = 0xA5
FIELDS = ("pos", "rot", "qpos", "qrot", "qcdage", "misc", "actions", "rewards")


def bits(t):
    return t.clone(memory_format=torch.contiguous_format).reshape(-1).view(torch.uint8)


def tensors(rec):
    d = dict(rec.states)
    d.update(actions=rec.actions, rewards=rec.rewards)
    return d


def patterned(kit, slabs, games, per_block):
    """a record whose every byte is PATTERN"""
    from skillshot_learning_amd import _capi
    rec = kit["ssa"].MatchRecord.allocate(slabs, games, _capi.default_config(), "cuda", per_block=per_block)
    refill(rec)
    return rec


def refill(rec):
    for t in tensors(rec).values():
        t.view(torch.uint8).fill_(PATTERN)
    rec.lengths.fill_(-1)


def snapshot(rec):
    return {k: t.clone() for k, t in tensors(rec).items()}


def assert_same_record(a, b):
    for k in FIELDS:
        assert torch.equal(bits(a[k]), bits(b[k])), k


_SNAPS = {}


def snap_reference(kit, n, reward):
    """the per-tick loop of test_match_gpu.loop_reference, snapshotting (once
    per case, shared, never modified): states [LIMIT + 1, n, w] — slab s of a
    game is its state after s ticks, kept while the game lives and at the tick
    it ends — actions [LIMIT, 2, n, 2], rewards [LIMIT, 2, n], lengths"""
    key = (n, reward)
    if key in _SNAPS:
        return _SNAPS[key]
    ref = loop_reference(kit, n, reward, False)
    k1, k2 = kit["kernels"]
    g = fresh_env(kit, n)
    g.load_state_dict(ref["start"])
    obs = ref["obs0"]
    states = {name: torch.zeros((LIMIT + 1, n, w), dtype=dt, device="cuda") for name, dt, w in kit["PLANES"]}
    actions = torch.zeros((LIMIT, 2, n, 2), device="cuda")
    rewards = torch.zeros((LIMIT, 2, n), device="cuda")
    lengths = torch.zeros(n, dtype=torch.int32, device="cuda")
    alive = torch.ones(n, dtype=torch.bool, device="cuda")
    for name in states:
        states[name][0] = getattr(g, name)
    t = 0
    while bool(alive.any()):
        act = torch.stack((k1(obs[0]), k2(obs[1])))
        out = g.step(act, obs=True, reward=reward, auto_reset=False)
        actions[t] = torch.where(alive[None, :, None], act, actions[t])
        rewards[t] = torch.where(alive[None], out["reward"], rewards[t])
        for name in states:
            states[name][t + 1] = torch.where(alive[:, None], getattr(g, name), states[name][t + 1])
        lengths += alive.int()
        alive = alive & ~out["done"].bool()
        obs = out["obs"]
        t += 1
    torch.cuda.synchronize()
    assert torch.equal(lengths, ref["lengths"]) and t == ref["iters"]
    _SNAPS[key] = dict(states=states, actions=actions, rewards=rewards, lengths=lengths)
    return _SNAPS[key]


def expected_record(snap, games, slab_lengths):
    """what a record of the games `games` must hold after a launch on a
    patterned record: the snapshot up to each row's length, PATTERN past it"""
    L = slab_lengths[games].long()
    out = {}
    for k in FIELDS:
        src = snap["states"][k][:, games] if k in snap["states"] else \
            (snap["actions"][:, :, games] if k == "actions" else snap["rewards"][:, :, games])
        S = src.shape[0]
        s = torch.arange(S, device="cuda")
        valid = (s[:, None] <= L[None]) if k in snap["states"] else (s[:, None] < L[None])
        valid = valid & (L[None] >= 1)
        pat = torch.empty_like(src)
        pat.view(torch.uint8).fill_(PATTERN)
        if k in snap["states"]:
            m = valid[:, :, None]
        elif k == "actions":
            m = valid[:, None, :, None]
        else:
            m = valid[:, None, :]
        out[k] = torch.where(m, src, pat)
    return out


CASES = [(228, 228), (228, 5), (37, 37), (37, 5), (32, 32), (32, 5), (1, 1)]


@pytest.mark.parametrize("reward", ["looking", "simple"])
@pytest.mark.parametrize("n,per", CASES, ids=[f"{n}-rec{p}" for n, p in CASES])
def test_record_equals_snapshotting_loop(kit, monkeypatch, n, per, reward):
    """228 games: 7 workgroups and a tail of 4; 37 recording 5: workgroup 0
    records part of its lanes, workgroup 1 none; 32: one workgroup; 1: a
    single game.  States s <= L, actions and rewards of every recorded row
    equal the loop's snapshots; every slab past L and every byte of an
    unrecorded region keep the pattern; the match's own outputs and the step
    counter are the plain launch's"""
    monkeypatch.setenv("SK_FWD16", "0")
    ref = loop_reference(kit, n, reward, False)
    snap = snap_reference(kit, n, reward)
    k1, k2 = kit["kernels"]
    ctrs = [int(k._ctr[0]) for k in kit["kernels"]]
    g = fresh_env(kit, n)
    g.load_state_dict(ref["start"])
    c0 = g.step_counter
    rec = patterned(kit, LIMIT + 1, torch.arange(per), per)
    m = g.act_match(k1, k2, ref["obs0"], n_ticks=LIMIT + 20, reward=reward, record=rec)
    torch.cuda.synchronize()
    assert m["record"] is rec and rec.ticks_run == LIMIT
    assert_same_match(kit, g, m, ref)
    T = int(m["lengths"].max())
    assert T == ref["iters"] and g.step_counter == c0 + T == ref["step_counter"]
    assert [int(k._ctr[0]) for k in kit["kernels"]] == ctrs
    assert torch.equal(rec.lengths, ref["lengths"][:per])
    assert_same_record(tensors(rec), expected_record(snap, rec.games, ref["lengths"]))
    for j in (0, per - 1):
        gm = rec.game(j)
        assert gm["length"] == int(ref["lengths"][j]) and gm["actions"].shape == (gm["length"], 2, 2)
    if (n, per) == (228, 228):
        rows = torch.arange(n, device="cuda")
        final = rec.states["misc"][rec.lengths.long(), rows, 1]
        w, ln = (final >> 24) & 0xFF, rec.lengths
        hit1, hit2, draws = int((w == 1).sum()), int((w == 2).sum()), int((w == 0).sum())
        print(f"{reward}: recorded hits on seat 1 / seat 2 / draws {hit1}/{hit2}/{draws}, shortest {int(ln.min())}")
        assert hit1 >= 3 and hit2 >= 3 and draws >= 3 and int(ln.min()) < 10
        assert torch.equal(w.long(), g.winner_id.long())


def test_record_in_chunks(kit, monkeypatch):
    """launches of 7 ticks with resume=True, the record continuing at the slab
    the earlier launches reached: the record of one launch, byte for byte (100
    games recording 40: workgroup 0 whole, workgroup 1 in part, the rest not)"""
    monkeypatch.setenv("SK_FWD16", "0")
    n, per = 100, 40
    ref = loop_reference(kit, n, "looking", False)
    k1, k2 = kit["kernels"]
    single = fresh_env(kit, n)
    single.load_state_dict(ref["start"])
    one = patterned(kit, LIMIT + 1, torch.arange(per), per)
    single.act_match(k1, k2, ref["obs0"], n_ticks=LIMIT, record=one)
    g = fresh_env(kit, n)
    g.load_state_dict(ref["start"])
    rec = patterned(kit, LIMIT + 1, torch.arange(per), per)
    m = g.act_match(k1, k2, ref["obs0"], n_ticks=7, record=rec)
    launches = 1
    while int(m["call_lengths"].max()) > 0:
        assert rec.ticks_run == min(7 * launches, LIMIT)
        m = g.act_match(k1, k2, m["obs"], n_ticks=7, out=m, resume=True, record=rec)
        launches += 1
        assert launches < 20
    torch.cuda.synchronize()
    assert launches == -(-ref["iters"] // 7) + 1
    assert_same_match(kit, g, m, ref)
    assert torch.equal(rec.lengths, one.lengths) and torch.equal(rec.lengths, ref["lengths"][:per])
    assert_same_record(tensors(rec), tensors(one))
    assert_same_record(tensors(one), expected_record(snap_reference(kit, n, "looking"), one.games, ref["lengths"]))


def test_record_under_capture(kit, monkeypatch):
    """one recording act_match captured on a side stream and replayed twice,
    each time from the reloaded start onto a re-patterned record: the eager
    record"""
    monkeypatch.setenv("SK_FWD16", "0")
    n, per = 37, 5
    ref = loop_reference(kit, n, "looking", False)
    k1, k2 = kit["kernels"]
    g = fresh_env(kit, n)
    g.load_state_dict(ref["start"])
    rec = patterned(kit, LIMIT + 1, torch.arange(per), per)
    bufs = g.act_match(k1, k2, ref["obs0"], n_ticks=LIMIT, record=rec)  # eager: the buffers, a warm launch
    torch.cuda.synchronize()
    eager = snapshot(rec)
    assert_same_record(eager, expected_record(snap_reference(kit, n, "looking"), rec.games, ref["lengths"]))
    g.load_state_dict(ref["start"])
    obs0 = ref["obs0"].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        g.sync_step_counter()
        with torch.cuda.graph(graph, stream=side):
            m = g.act_match(k1, k2, obs0, n_ticks=LIMIT, out=bufs, record=rec)
    torch.cuda.synchronize()
    for _ in range(2):
        refill(rec)
        for t in (m["lengths"], m["returns"], m["obs"]):
            t.zero_()
        g.load_state_dict(ref["start"])
        with torch.cuda.stream(side):
            g.sync_step_counter()
            graph.replay()
        torch.cuda.synchronize()
        assert_same_match(kit, g, m, ref)
        assert_same_record(tensors(rec), eager)
        assert torch.equal(rec.lengths, ref["lengths"][:per])


def test_record_boards_equal_the_cpu_painter(kit, monkeypatch):
    """boards(j) on the device (one render launch per row) against the CPU
    backend's painter on the same states, the recorded rows of the 37-game case"""
    monkeypatch.setenv("SK_FWD16", "0")
    n, per = 37, 5
    ref = loop_reference(kit, n, "looking", False)
    g = fresh_env(kit, n)
    g.load_state_dict(ref["start"])
    rec = g.act_match(*kit["kernels"], ref["obs0"], n_ticks=LIMIT, record=per)["record"]
    host = rec.cpu()
    assert host.device.type == "cpu" and rec.device.type == "cuda"
    for j in range(per):
        dev_boards = rec.boards(j)
        assert dev_boards.is_cuda and dev_boards.shape == (int(rec.lengths[j]) + 1, 250, 250)
        assert torch.equal(dev_boards.cpu(), host.boards(j)), j
        assert int(dev_boards[0].sum()) > 0


# ---------------------------------------------------------------- league
@pytest.fixture(scope="module")
def kit3(kit):
    from skillshot_learning_amd.actor_kernel import ActorKernel32
    from test_match_cpu import turning_actor
    nets = [turning_actor(s).cuda() for s in lgt.ACTOR_SEEDS]
    kernels = [ActorKernel32(m, seed=5 + k) for k, m in enumerate(nets)]
    return dict(kit, nets=nets, kernels=kernels)


def test_league_record_equals_match_records(kit3, monkeypatch):
    """three actors, blocks of 64 with 40 live games each (two workgroups per
    pairing, 24 pad games), 3 games recorded per pairing: rows 3p .. 3p + 2
    are the record of act_match between pairing p's actors; then a pairing
    pointing outside the table records nothing and leaves the others alone"""
    monkeypatch.setenv("SK_FWD16", "0")
    kit, games, block, per, bad = kit3, 40, 64, 3, 3
    P = len(lgt.PAIRS)
    ref = lgt.match_reference(kit, games, "looking")
    g = kit["ssa"].VecSkillshotGame(games, device="cuda", seed=ENV_SEED, tick_limit=LIMIT)
    want = {k: [] for k in FIELDS}
    want_len = []
    for i, j in lgt.PAIRS:
        g.load_state_dict(ref["start"])
        r = patterned(kit, LIMIT + 1, torch.arange(per), per)
        g.act_match(kit["kernels"][i], kit["kernels"][j], ref["obs0"], n_ticks=LIMIT, record=r)
        for k, t in tensors(r).items():
            want[k].append(t)
        want_len.append(r.lengths)
    cat = {k: torch.cat(v, 1 if k in ("pos", "rot", "qpos", "qrot", "qcdage", "misc") else 2) for k, v in want.items()}
    lg, sd, obs = lgt.league_env(kit, ref, games, block)
    rows = (torch.arange(P)[:, None] * block + torch.arange(per)[None]).reshape(-1)
    rec = patterned(kit, LIMIT + 1, rows, per)
    m = lg.act_league(kit["kernels"], lgt.PAIRS, block, obs, n_ticks=LIMIT, record=rec)
    torch.cuda.synchronize()
    lgt.assert_same_league(kit, lg, m, ref, sd, games, block)
    assert m["record"] is rec and rec.pairs == [pr for pr in lgt.PAIRS for _ in range(per)]
    assert torch.equal(rec.lengths, torch.cat(want_len)) and int(rec.lengths.min()) >= 1
    assert_same_record(tensors(rec), cat)
    assert len({tuple(bits(t).tolist()) for t in want["actions"]}) >= 5  # the pairings' records differ

    lg.load_state_dict(sd)
    m["pairs"][bad, 1] = len(kit["kernels"])
    refill(rec)
    m = lg.act_league(kit["kernels"], lgt.PAIRS, block, obs, n_ticks=LIMIT, out=m, record=rec)
    torch.cuda.synchronize()
    lgt.assert_same_league(kit, lg, m, ref, sd, games, block, skip=(bad,))
    got = tensors(rec)
    for k in FIELDS:
        dim = 1 if k in rec.states else 2
        sl = [slice(None)] * got[k].dim()
        sl[dim] = slice(bad * per, (bad + 1) * per)
        skipped = got[k][tuple(sl)]
        assert bool((bits(skipped) == PATTERN).all()), k  # the refused pairing wrote nothing
        keep = torch.ones(P * per, dtype=torch.bool, device="cuda")
        keep[bad * per:(bad + 1) * per] = False
        assert torch.equal(bits(got[k].movedim(dim, 0)[keep]), bits(cat[k].movedim(dim, 0)[keep])), k
    assert rec.lengths[bad * per:(bad + 1) * per].tolist() == [0] * per


# ---------------------------------------------------------------- the learner's two paths
def same_records(a, b):
    assert (a.rows, a.slabs, a.per_block, a.pairs) == (b.rows, b.slabs, b.per_block, b.pairs)
    assert torch.equal(a.lengths, b.lengths) and torch.equal(a.games, b.games)
    assert_same_record(tensors(a), tensors(b))


def test_learner_records_kernel_equals_loop(kit3, monkeypatch):
    """evaluate(record=4) and league(record=2): the one-launch kernels'
    records and the per-tick loop's (SK_MATCH_KERNEL=0, SK_LEAGUE_KERNEL=0),
    whole tensors, and the results around them"""
    monkeypatch.setenv("SK_FWD16", "0")
    kit = kit3
    L = lgt.gpu_learner(kit)
    with torch.no_grad():
        L.model_actor.load_state_dict(kit["nets"][0].state_dict())
    ev, lg = {}, {}
    for flag in ("1", "0"):
        monkeypatch.setenv("SK_MATCH_KERNEL", flag)
        monkeypatch.setenv("SK_LEAGUE_KERNEL", flag)
        ev[flag] = L.evaluate(opponent=kit["nets"][1], games=100, tick_limit=LIMIT, seed=ENV_SEED, record=4)
        lg[flag] = L.league([None, kit["nets"][1], kit["nets"][2]], games=40, tick_limit=LIMIT, seed=ENV_SEED,
                            record=2)
    ra, rb = ev["1"].pop("records"), ev["0"].pop("records")
    assert ev["1"] == ev["0"] and len(ra) == len(rb) == 2
    for a, b in zip(ra, rb):
        same_records(a, b)
        assert a.device.type == "cuda" and a.rows == 4 and int(a.lengths.min()) >= 1
    for name in ra[0].states:
        assert torch.equal(bits(ra[0].states[name][0]), bits(ra[1].states[name][0])), name  # both legs' start
    la, lb = lg["1"].pop("record"), lg["0"].pop("record")
    assert lg["1"] == lg["0"]
    same_records(la, lb)
    assert la.rows == 12 and la.pairs[:4] == [(0, 1), (0, 1), (0, 2), (0, 2)] and la.games.tolist() == [0, 1] * 6
    monkeypatch.setenv("SK_MATCH_KERNEL", "1")
    plain = L.evaluate(opponent=kit["nets"][1], games=100, tick_limit=LIMIT, seed=ENV_SEED)
    assert plain == ev["1"]
