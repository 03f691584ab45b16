"""Match statistics on the GPU: the one-launch league that tallies them in
wave 0's registers (sk_env_act_league_stats) against the per-tick path
(k_stats_tick before every step), word for word; k_stats_tick against the CPU
backend's sk_env_stats_tick on the same states; and the calls without
statistics returning what they returned."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GAMES, BLOCK, LIMIT = 40, 64, 48  # a padded block (24 pad games, two workgroups per pairing); three shots and more per seat
ENV_SEED = 6
ACTOR_SEEDS = (23, 27)            # test_league_gpu's: they turn, move and hit


@pytest.fixture(scope="module")
def kit():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import skillshot_learning_amd as ssa
    from skillshot_learning_amd import _capi, learner
    from test_match_cpu import turning_actor
    nets = [turning_actor(s).cuda() for s in ACTOR_SEEDS]
    return dict(ssa=ssa, learner=learner, nets=nets, capi=_capi)


def bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype != torch.bool else t


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


def paths(monkeypatch, fn):
    """fn() on the one-launch path, then on the per-tick path"""
    out = []
    for flag in ("1", "0"):
        monkeypatch.setenv("SK_LEAGUE_KERNEL", flag)
        monkeypatch.setenv("SK_MATCH_KERNEL", flag)
        out.append(fn())
    monkeypatch.setenv("SK_LEAGUE_KERNEL", "1")
    monkeypatch.setenv("SK_MATCH_KERNEL", "1")
    return out


def test_one_launch_equals_the_per_tick_path_word_for_word(kit, monkeypatch):
    """net-net, net-bot and bot-bot pairings, 40 of 64 games per block: every
    word of the raw buffers, on_target included (same primitive, same states);
    the reported tables; the pad games' words and the two carry planes left as
    initialised; and with record=8 the record of the launch without stats"""
    monkeypatch.setenv("SK_FWD16", "0")
    capi = kit["capi"]
    L = gpu_learner(kit)
    actors = [None, kit["nets"][1], "chaser", "still"]
    fused, loop = paths(monkeypatch, lambda: L.league(actors, games=GAMES, tick_limit=LIMIT, seed=ENV_SEED, stats=True))
    raw_f, raw_l = fused.pop("stats_raw"), loop.pop("stats_raw")
    torch.cuda.synchronize()
    assert raw_f.shape == raw_l.shape == (8, 2, 12, GAMES) and raw_f.dtype == torch.int32
    for k, name in enumerate(capi.STAT_NAMES):
        assert torch.equal(raw_f[k], raw_l[k]), name
    assert fused == loop  # nan-free: every pairing played ticks
    r = raw_f.long()
    print("shots", r[0].sum().item(), "on_target", r[2].sum().item(), "under_fire", r[3].sum().item(), "at_wall",
          r[4].sum().item(), "path", r[5].sum().item(), "hits",
          sum(map(sum, fused["seat_wins"])) + sum(map(sum, fused["seat_losses"])))
    # the games exercise every counter, and some end by a hit before the limit
    assert int(r[0].max()) >= 3 and all(int(r[k].sum()) > 0 for k in (0, 1, 2, 3, 5, 6, 7))
    assert sum(map(sum, fused["seat_wins"])) + sum(map(sum, fused["seat_losses"])) >= 20
    assert int(r[7].max()) < capi.SK_STAT_FAR
    assert fused["actor_stats"]["path"][3] == 0.0 and fused["actor_stats"]["path"][2] > 0.0
    # the launch's own buffer: pad games and the carry planes as new_stats left them
    lg = next(iter(L._league_envs.values()))
    buf = lg._league_bufs["stats"].view(10, 2, 12, BLOCK)
    init = lg.new_stats().view(10, 2, 12, BLOCK)
    assert torch.equal(buf[..., GAMES:], init[..., GAMES:]) and torch.equal(buf[8:], init[8:])
    assert torch.equal(buf[:8, ..., :GAMES], raw_f)
    # record=8 beside the statistics: the record of the call without them, and the same tallies again
    with_rec = L.league(actors, games=GAMES, tick_limit=LIMIT, seed=ENV_SEED, stats=True, record=8)
    plain_rec = L.league(actors, games=GAMES, tick_limit=LIMIT, seed=ENV_SEED, record=8)
    torch.cuda.synchronize()
    assert with_rec["record"].rows == 12 * 8
    assert_same_record(with_rec.pop("record"), plain_rec.pop("record"))
    assert torch.equal(with_rec.pop("stats_raw"), raw_f)
    assert with_rec == fused
    for key in ("stats", "opponent_stats", "actor_stats"):
        with_rec.pop(key)
    assert with_rec == plain_rec


def test_evaluate_with_stats_fused_equals_the_loop_and_changes_no_other_number(kit, monkeypatch):
    monkeypatch.setenv("SK_FWD16", "0")
    L = gpu_learner(kit)
    for opp in (kit["nets"][1], "chaser"):
        fused, loop = paths(monkeypatch, lambda: L.evaluate(opp, games=GAMES, tick_limit=LIMIT, seed=ENV_SEED,
                                                            stats=True))
        plain = L.evaluate(opp, games=GAMES, tick_limit=LIMIT, seed=ENV_SEED)  # act_match for the net: no statistics
        torch.cuda.synchronize()
        for a, b in zip(fused.pop("stats_raw"), loop.pop("stats_raw")):
            assert a.shape == (8, 2, GAMES) and torch.equal(a, b)
        assert fused == loop
        fused.pop("stats")
        for leg in fused["legs"]:
            leg.pop("stats")
        assert fused == plain and "stats" not in plain


def test_stats_tick_equals_the_cpu_backend(kit):
    """40 games (80 lanes: a partial workgroup), 48 ticks of random actions,
    ended games masked out; one rotation past sincos_bf's range"""
    n = GAMES
    c, g = [kit["ssa"].VecSkillshotGame(n, device=d, seed=11, env_offset=5, tick_limit=LIMIT) for d in ("cpu", "cuda")]
    c.reset(random_positions=True)
    st = c.state_dict()
    st["rot"][3] = (1.0e7, -2.5e6)
    c.load_state_dict(st)
    g.load_state_dict(st)
    sc, sg = c.new_stats(), g.new_stats()
    lived = 0
    for t in range(LIMIT):
        alive = c.game_live & (c.ticks < c.tick_limit)
        lived += int(alive.sum())
        c.stats_tick(sc, alive)
        g.stats_tick(sg, alive.cuda())
        act = c.gen_random_actions(1)[0]
        c.step(act, obs=False, reward="looking", auto_reset=False)
        g.step(act.cuda(), obs=False, reward="looking", auto_reset=False)
    torch.cuda.synchronize()
    assert torch.equal(sg.cpu(), sc)
    for name in ("pos", "rot", "qpos", "misc"):
        assert torch.equal(bits(getattr(g, name).cpu()), bits(getattr(c, name))), name
    s = sc.long()
    assert n * 10 < lived < n * LIMIT  # some games ended before the limit and stopped counting
    assert int(s[0].sum()) > 2 * n and int(s[5].sum()) > 0 and int(s[7].max()) < kit["capi"].SK_STAT_FAR
    with pytest.raises(ValueError):
        g.stats_tick(sc, alive.cuda())  # a host buffer for a device env


def test_net_only_league_without_stats_returns_what_it_returned(kit, monkeypatch):
    monkeypatch.setenv("SK_FWD16", "0")
    L = gpu_learner(kit)
    fused, loop = paths(monkeypatch, lambda: L.league([None, kit["nets"][1]], games=GAMES, tick_limit=LIMIT,
                                                      seed=ENV_SEED))
    assert fused == loop and "stats" not in fused
    assert sum(map(sum, fused["seat_wins"])) + sum(map(sum, fused["seat_losses"])) >= 1
