"""Match statistics without a GPU: the CPU backend's sk_env_stats_tick, called
by evaluate's and league's per-tick loop, against the plain-Python restatement
(stats_ref.py) over full match records; the reported values against the raw
words; the result's shapes; that asking for statistics changes no other
number; and the refusals."""
import math

import numpy as np
import pytest
import torch

import skillshot_learning_amd as ssa
import stats_ref
from skillshot_learning_amd import _capi
from skillshot_learning_amd.learner import STAT_REPORT
from test_match_cpu import cpu_learner

FLAGS = ("in_flight", "on_target", "under_fire", "at_wall")


def without_stats(d):
    d = {k: v for k, v in d.items() if k not in ("stats", "opponent_stats", "actor_stats", "stats_raw", "records",
                                                 "record")}
    if "legs" in d:
        d["legs"] = [without_stats(leg) for leg in d["legs"]]
    return d


@pytest.fixture(scope="module")
def chaser_eval():
    L = cpu_learner()
    return L, L.evaluate(opponent="chaser", games=24, tick_limit=40, stats=True, record=24)


def test_every_word_of_every_game_and_seat_equals_the_restatement(chaser_eval):
    _, res = chaser_eval
    assert _capi.STAT_NAMES == stats_ref.NAMES and _capi.SK_N_STATS == 8
    assert len(res["stats_raw"]) == len(res["records"]) == 2
    cases = close = compared = 0
    for raw, rec in zip(res["stats_raw"], res["records"]):
        assert raw.shape == (8, 2, 24) and raw.dtype == torch.int32 and rec.rows == 24
        assert int(rec.lengths.min()) >= 1
        want, undecided, n, c = stats_ref.of_record(rec)
        cases, close = cases + n, close + c
        got = raw.numpy().astype(np.int64)
        for k, name in enumerate(stats_ref.NAMES):
            if name == "on_target":
                keep = ~undecided
                compared += int(keep.sum())
                assert np.array_equal(got[k][keep], want[k][keep]), name
            else:
                assert np.array_equal(got[k], want[k]), name
    print("on_target: too close to call", close, "of", cases, "cases;", compared, "(game, seat) compared")
    assert close <= 0.01 * cases and compared >= 0.9 * 2 * 2 * 24
    # the games do something: shots are fired, projectiles fly, the chaser walks
    tot = sum(r.numpy().astype(np.int64).sum(-1) for r in res["stats_raw"])
    assert tot[0].min() > 0 and tot[1].min() > 0 and tot[5].max() > 0


def test_reported_values_follow_the_raw_words(chaser_eval):
    _, res = chaser_eval
    sums = []
    for k, (leg, raw, rec) in enumerate(zip(res["legs"], res["stats_raw"], res["records"])):
        raw = raw.numpy().astype(np.int64)
        ticks = int(rec.lengths.sum())
        assert ticks == round(leg["mean_ticks"] * 24)
        for who, seat in (("mine", k), ("theirs", 1 - k)):  # leg k + 1 has the learner in seat k + 1
            d, w = leg["stats"][who], raw[:, seat]
            assert tuple(d) == STAT_REPORT
            assert d["shots"] == w[0].sum() and isinstance(d["shots"], int)
            for name in FLAGS + ("path",):
                assert d[name] == w[stats_ref.NAMES.index(name)].sum() / ticks, name
            assert d["mean_distance"] == w[6].sum() / ticks and d["closest"] == w[7].sum() / 24
            sums.append((who, w.sum(-1), ticks))
    for who in ("mine", "theirs"):
        w = sum(s for n, s, _ in sums if n == who)
        ticks = sum(t for n, _, t in sums if n == who)
        d = res["stats"][who]
        assert d["shots"] == w[0] and d["at_wall"] == w[4] / ticks and d["mean_distance"] == w[6] / ticks
        assert d["closest"] == w[7] / 48
    for d in (res["stats"]["mine"], res["stats"]["theirs"]):
        assert all(0.0 <= d[name] <= 1.0 for name in FLAGS) and 0 < d["closest"] <= d["mean_distance"]
    # the chaser walks towards its opponent, a net with small outputs hardly moves
    assert res["stats"]["theirs"]["path"] > 0


def test_league_tables_shapes_and_sanity():
    L = cpu_learner()
    K, n = 3, 8
    lg = L.league([None, "aimer", "still"], games=n, tick_limit=30, stats=True)
    for key in ("stats", "opponent_stats"):
        assert tuple(lg[key]) == STAT_REPORT
        for name in STAT_REPORT:
            t = np.array(lg[key][name])
            assert t.shape == (K, K) and np.all(np.diag(t) == 0), (key, name)
    assert tuple(lg["actor_stats"]) == STAT_REPORT
    assert all(len(lg["actor_stats"][name]) == K for name in STAT_REPORT)
    raw = lg["stats_raw"].numpy().astype(np.int64)
    assert raw.shape == (8, 2, K * (K - 1), n)
    pairs = [(i, j) for i in range(K) for j in range(K) if i != j]
    ticks = np.rint(np.array(lg["mean_ticks"]) * n)
    off = ~np.eye(K, dtype=bool)
    # actor_stats is the sum of the two seatings: counts add, shares and per-tick values by their ticks
    shots = np.array(lg["stats"]["shots"]).sum(1) + np.array(lg["opponent_stats"]["shots"]).sum(0)
    assert np.array_equal(shots, np.array(lg["actor_stats"]["shots"]))
    played = ticks.sum(1) + ticks.sum(0)
    for name in FLAGS + ("path", "mean_distance"):
        k = STAT_REPORT.index(name)
        total = np.zeros(K)
        for q, (i, j) in enumerate(pairs):
            total[i] += raw[k, 0, q].sum()
            total[j] += raw[k, 1, q].sum()
            assert lg["stats"][name][i][j] == raw[k, 0, q].sum() / ticks[i, j], name
            assert lg["opponent_stats"][name][i][j] == raw[k, 1, q].sum() / ticks[i, j], name
        assert np.array_equal(total / played, np.array(lg["actor_stats"][name])), name
    # still never moves; an aimer faces its opponent more often than still does
    assert lg["actor_stats"]["path"][2] == 0.0
    assert np.all(np.array(lg["stats"]["path"])[2] == 0) and np.all(np.array(lg["opponent_stats"]["path"])[:, 2] == 0)
    assert lg["actor_stats"]["on_target"][1] > lg["actor_stats"]["on_target"][2]
    assert np.all(np.array(lg["stats"]["mean_distance"])[off] > 0)
    # both seats of a game see the same distances
    assert lg["stats"]["mean_distance"] == lg["opponent_stats"]["mean_distance"]
    assert lg["stats"]["closest"] == lg["opponent_stats"]["closest"]


def test_every_other_number_is_the_same_with_and_without_stats(chaser_eval):
    L, res = chaser_eval
    plain = L.evaluate(opponent="chaser", games=24, tick_limit=40)
    assert "stats" not in plain and "stats_raw" not in plain and without_stats(res) == plain
    mirror = L.evaluate(opponent=None, games=24, tick_limit=40, reward="simple")
    assert without_stats(L.evaluate(opponent=None, games=24, tick_limit=40, reward="simple", stats=True)) == mirror
    a = L.league([None, "aimer", "still"], games=8, tick_limit=30)
    b = L.league([None, "aimer", "still"], games=8, tick_limit=30, stats=True, record=2)
    assert "stats" not in a and b["record"].rows == 12 and without_stats(b) == a


def test_a_game_that_starts_ended_keeps_closest_out_of_the_mean():
    L = cpu_learner()
    g = L._eval_env(8, 30, None)
    g.step_counter = 0
    g.reset(random_positions=True)
    g.misc[2, 1] &= ~0x00FF0000  # game 2 is not live: it plays no tick
    mine, bot = L._match_actor(None), L._match_actor("aimer")
    row = L._match_leg(g, mine, bot, 1, 30, "looking", False, stats=True).numpy()
    raw = L._stats_raw.numpy().astype(np.int64)[:, :, 0]
    assert np.all(raw[:7, :, 2] == 0) and np.all(raw[7, :, 2] == _capi.SK_STAT_FAR)
    others = [i for i in range(8) if i != 2]
    assert np.all(raw[7][:, others] < _capi.SK_STAT_FAR) and np.all(raw[0][:, others] >= 1)
    from skillshot_learning_amd.learner import _stats_dict
    d = _stats_dict(row[6:16])
    assert row[6 + 8] == 7 and d["closest"] == raw[7, 0, others].sum() / 7
    # no game plays at all: nothing to average
    g.reset(random_positions=True)
    g.misc[:, 1] &= ~0x00FF0000
    d = _stats_dict(L._match_leg(g, mine, bot, 1, 30, "looking", False, stats=True).numpy()[6:16])
    assert d["shots"] == 0 and math.isnan(d["closest"]) and math.isnan(d["in_flight"])


def test_overflow_and_wrong_buffers_are_refused():
    cfg = _capi.default_config()
    limit = (2 ** 31 - 1) // max(cfg.board_w, cfg.board_h)
    ok = ssa.VecSkillshotGame(32, device="cpu", tick_limit=limit)
    big = ssa.VecSkillshotGame(32, device="cpu", tick_limit=limit + 1)
    s = ok.new_stats()
    assert s.shape == (10, 2, 32) and s.dtype == torch.int32
    assert torch.all(s[7] == _capi.SK_STAT_FAR) and torch.all(s[8] == _capi.SK_STAT_NO_PREV)
    assert torch.all(s[:7] == 0) and torch.all(s[9] == 0)
    alive = torch.ones(32, dtype=torch.uint8)
    with pytest.raises(ValueError):
        big.new_stats()
    with pytest.raises(ValueError):
        big.stats_tick(s, alive)
    for bad in (torch.zeros((8, 2, 32), dtype=torch.int32), torch.zeros((10, 2, 32), dtype=torch.int64),
                torch.zeros((10, 2, 31), dtype=torch.int32), torch.zeros((10, 32, 2), dtype=torch.int32).transpose(1, 2),
                None):
        with pytest.raises(ValueError):
            ok.stats_tick(bad, alive)
    with pytest.raises(ValueError):
        ok.new_stats(out=torch.zeros((8, 2, 32), dtype=torch.int32))
    with pytest.raises(ValueError):
        ok.stats_tick(s, alive[:31])
    lib = ssa.load_library()
    a8 = np.ones(32, np.uint8)
    buf = np.zeros(10 * 2 * 32 + 1, np.int32)
    assert lib.sk_env_stats_tick(ok._h, None, buf.ctypes.data, None) == _capi.SK_EINVAL
    assert lib.sk_env_stats_tick(ok._h, a8.ctypes.data, None, None) == _capi.SK_EINVAL
    assert lib.sk_env_stats_tick(None, a8.ctypes.data, buf.ctypes.data, None) == _capi.SK_EINVAL
    assert lib.sk_env_stats_tick(ok._h, a8.ctypes.data, buf.ctypes.data + 2, None) == _capi.SK_EINVAL
    assert lib.sk_env_stats_tick(ok._h, a8.ctypes.data, buf.ctypes.data, None) == _capi.SK_OK
    # the one-launch symbol: the range check comes before the backend's (both handles are CPU ones)
    nets, pairs = np.zeros((1, 2), np.uint64), np.zeros((1, 2), np.int32)
    obs2 = torch.zeros((2, 2, 32, 12))
    ret, ln = np.zeros((2, 32), np.float32), np.zeros(32, np.int32)

    def launch(g, stats_ptr, tick_limit):
        rc = lib.sk_env_act_league_stats(g._h, nets.ctypes.data, 1, pairs.ctypes.data, 1, 32, obs2.data_ptr(),
                                         ret.ctypes.data, ln.ctypes.data, None, 4, 0, tick_limit, stats_ptr, None, None)
        return rc, lib.sk_last_error().decode()

    rc, msg = launch(big, buf.ctypes.data, limit + 1)
    assert rc == _capi.SK_EINVAL and "int32" in msg
    rc, msg = launch(ok, None, limit)
    assert rc == _capi.SK_EINVAL and "stats" in msg
    rc, msg = launch(ok, buf.ctypes.data, limit)
    assert rc == _capi.SK_EINVAL and "GPU backend" in msg
    for name in ("sk_env_act_league_stats", "sk_env_stats_tick"):
        assert name in _capi.EXPORTS and getattr(lib, name) is not None
    assert lib.sk_abi_version() == 13


def test_stats_tick_with_nobody_alive_changes_nothing():
    g = ssa.VecSkillshotGame(16, device="cpu", seed=9, tick_limit=60)
    g.reset(random_positions=True)
    g.rollout_random(7)
    s = g.new_stats()
    s.copy_(torch.randint(-5, 500, s.shape, dtype=torch.int32, generator=torch.Generator().manual_seed(1)))
    before, state = s.clone(), g.state_dict()
    assert g.stats_tick(s, torch.zeros(16, dtype=torch.uint8)) is s and torch.equal(s, before)
    half = (torch.arange(16) % 2).to(torch.uint8)
    g.stats_tick(s, half)
    assert torch.equal(s[:, :, 0::2], before[:, :, 0::2]) and not torch.equal(s[:, :, 1::2], before[:, :, 1::2])
    after = g.state_dict()
    assert all(np.array_equal(np.asarray(state[k]), np.asarray(after[k])) for k in state)  # advances nothing
