"""Match records without a GPU: the two recording entry points' argument
checks, SkillshotLearner.evaluate(record=) and league(record=) on the CPU
backend (the per-tick loop path fills the record), the record against a host
replay of its own actions (trace_game), its boards against the reference
painter, and persistence."""
import ctypes

import numpy as np
import pytest
import torch

import skillshot_learning_amd as ssa
from skillshot_learning_amd import _capi, persist
from skillshot_learning_amd.game import rasterize_board
from skillshot_learning_amd.vec_env import PLANES
from test_match_cpu import GAMES, LIMIT, cpu_learner, turning_actor

REC = 6


def bits(t):
    return t.clone(memory_format=torch.contiguous_format).reshape(-1).view(torch.uint8)


@pytest.fixture(scope="module")
def played():
    """one evaluate with and without a record, shared (never modified)"""
    L = cpu_learner()
    opp = turning_actor(12)
    plain = L.evaluate(opponent=opp, games=GAMES, tick_limit=LIMIT)
    res = L.evaluate(opponent=opp, games=GAMES, tick_limit=LIMIT, record=REC)
    return dict(L=L, opp=opp, plain=plain, res=res)


# ---------------------------------------------------------------- the C ABI
class RecBufs:
    """host buffers of a valid sk_match_record (the checks run before any launch and read no memory)"""

    def __init__(self, slabs, rows, per_block, slab0=0):
        n = slabs * rows
        self.keep = [np.zeros(16 * n + 64, dtype=np.uint8) for _ in range(8)]
        p = [b.ctypes.data for b in self.keep]
        assert all(a % 16 == 0 for a in p)
        self.rec = _capi.SkMatchRecord(_capi.SkStateView(n, *p[:6]), p[6], p[7], slabs, rows, per_block, slab0)

    def with_(self, **kw):
        r = _capi.SkMatchRecord()
        ctypes.memmove(ctypes.byref(r), ctypes.byref(self.rec), ctypes.sizeof(r))
        for k, v in kw.items():
            if k in ("pos", "rot", "qpos", "qrot", "qcdage", "misc", "n_envs"):
                setattr(r.states, k, v)
            else:
                setattr(r, k, v)
        return r


def refusals(call, bufs, block, n_ticks):
    """every refusal of a recording entry point the record itself can cause: (the record, a word of the message)"""
    r = bufs.rec
    cases = [(None, b"rec is NULL")]
    for plane in ("pos", "rot", "qpos", "qrot", "qcdage", "misc"):
        cases.append((bufs.with_(**{plane: None}), b"NULL"))
        cases.append((bufs.with_(**{plane: getattr(r.states, plane) + 4}), b"8-byte"))
    cases += [(bufs.with_(actions=None), b"NULL"),
              (bufs.with_(actions=r.actions + 2), b"4-byte"),
              (bufs.with_(rewards=r.rewards + 2), b"4-byte"),
              (bufs.with_(per_block=0), b"per_block"),
              (bufs.with_(per_block=block + 1), b"per_block"),
              (bufs.with_(rows=r.rows + 1), b"rows"),
              (bufs.with_(n_envs=r.states.n_envs + 1), b"n_envs"),
              (bufs.with_(slabs=r.slabs + 1), b"n_envs"),
              (bufs.with_(slab0=-1), b"slab0"),
              (bufs.with_(slab0=r.slabs - n_ticks), b"slab0 + n_ticks"),
              (bufs.with_(slab0=1), b"slab0 + n_ticks")]
    lib = ssa.load_library()
    for rec, word in cases:
        rc = call(rec)
        msg = lib.sk_last_error()
        assert rc == _capi.SK_EINVAL and word in msg, (word, msg)
    rc = call(bufs.rec)  # everything in order: the CPU backend itself is refused
    assert rc == _capi.SK_EINVAL and b"GPU" in lib.sk_last_error()


def test_recording_entry_points_resolve_and_refuse_bad_arguments():
    """sk_env_act_match_rec / sk_env_act_league_rec are new symbols of ABI 13;
    each refusal include/skillshot.h lists answers SK_EINVAL with a message,
    before any launch (so a CPU-backend handle shows them all)"""
    lib = ssa.load_library()
    assert lib.sk_abi_version() == _capi.ABI_VERSION == 13
    assert "sk_env_act_match_rec" in _capi.EXPORTS and "sk_env_act_league_rec" in _capi.EXPORTS
    assert lib.sk_env_act_match_rec is not None and lib.sk_env_act_league_rec is not None
    buf = (ctypes.c_float * 8192)()
    ln = (ctypes.c_int32 * 64)()
    T = 10

    # the match: 8 games, 4 of them recorded
    h = ctypes.c_void_p()
    assert lib.sk_env_create(ctypes.byref(h), 8, 0, 7, -1, None) == _capi.SK_OK
    bufs = RecBufs(T + 1, 4, 4)

    def match(rec, returns=buf, lengths=ln, n_ticks=T):
        return lib.sk_env_act_match_rec(h, buf, buf, buf, buf, buf, returns, lengths, None, n_ticks, 0, 2000,
                                        None if rec is None else ctypes.byref(rec), None)

    refusals(match, bufs, 8, T)
    # two faults: the record, and a bad argument ahead of it, are reported ahead of the CPU backend
    assert match(bufs.with_(per_block=0)) == _capi.SK_EINVAL
    assert b"per_block" in lib.sk_last_error() and b"GPU" not in lib.sk_last_error()
    assert match(bufs.with_(per_block=0), lengths=ctypes.c_void_p(ctypes.addressof(ln) + 1)) == _capi.SK_EINVAL
    assert b"aligned" in lib.sk_last_error()
    assert match(bufs.rec, returns=None) == _capi.SK_EINVAL and b"returns" in lib.sk_last_error()
    assert match(bufs.with_(rewards=None), returns=None) == _capi.SK_EINVAL and b"GPU" in lib.sk_last_error()
    assert match(bufs.rec, lengths=None) == _capi.SK_EINVAL and b"lengths" in lib.sk_last_error()  # the plain twin's
    assert match(bufs.rec, n_ticks=0) == _capi.SK_EINVAL and b"n_ticks" in lib.sk_last_error()
    assert lib.sk_env_act_match_rec(None, buf, buf, buf, buf, buf, buf, ln, None, T, 0, 2000,
                                    ctypes.byref(bufs.rec), None) == _capi.SK_EINVAL
    assert lib.sk_env_destroy(h) == _capi.SK_OK

    # the league: 2 pairings of 32 games, 3 recorded of each
    h = ctypes.c_void_p()
    assert lib.sk_env_create(ctypes.byref(h), 64, 0, 7, -1, None) == _capi.SK_OK
    bufs = RecBufs(T + 1, 6, 3)
    nets = (ctypes.c_uint64 * 4)()
    pairs = (ctypes.c_int32 * 4)()

    def league(rec, block=32, n_pairs=2, tables=(nets, pairs)):
        return lib.sk_env_act_league_rec(h, tables[0], 2, tables[1], n_pairs, block, buf, buf, ln, None, T, 0, 2000,
                                         None if rec is None else ctypes.byref(rec), None)

    refusals(league, bufs, 32, T)
    assert league(bufs.rec, block=33) == _capi.SK_EINVAL and b"block" in lib.sk_last_error()  # the plain twin's
    assert league(bufs.rec, n_pairs=1) == _capi.SK_EINVAL and b"n_pairs * block" in lib.sk_last_error()
    assert league(bufs.rec, tables=(None, pairs)) == _capi.SK_EINVAL and b"table" in lib.sk_last_error()
    assert lib.sk_env_destroy(h) == _capi.SK_OK


def test_act_match_record_needs_the_gpu_backend():
    g = ssa.VecSkillshotGame(4, device="cpu")
    with pytest.raises(ssa.SkillshotError):
        g.act_match(None, None, g.observe()[0], record=2)


# ---------------------------------------------------------------- evaluate
def test_evaluate_record_leaves_the_tallies_alone(played):
    res = dict(played["res"])
    recs = res.pop("records")
    assert res == played["plain"] and "records" not in played["plain"]
    assert len(recs) == 2 and all(isinstance(r, ssa.MatchRecord) for r in recs)
    for r in recs:
        assert r.rows == len(r) == REC and r.slabs == LIMIT + 1 and r.games.tolist() == list(range(REC))
        assert r.actions.shape == (LIMIT, 2, REC, 2) and r.rewards.shape == (LIMIT, 2, REC)
        assert r.pairs is None and r.device.type == "cpu" and r.cpu() is r
    with pytest.raises(ValueError):
        played["L"].evaluate(opponent=None, games=GAMES, tick_limit=LIMIT, record=GAMES + 1)
    with pytest.raises(TypeError):
        played["L"].evaluate(opponent=None, games=GAMES, tick_limit=LIMIT, record=True)


def test_record_is_the_replay_of_its_own_actions(played):
    """every row: trace_game from slab 0 on the recorded actions gives slabs
    1 .. L bit for bit; lengths are the final states' ticks; the final state
    is over (hit, or at the limit); both legs start from the same states"""
    g = ssa.VecSkillshotGame(1, device="cpu", tick_limit=LIMIT)
    a, b = played["res"]["records"]
    for name, _, _ in PLANES:
        assert torch.equal(bits(a.states[name][0]), bits(b.states[name][0])), name
    assert not torch.equal(bits(a.actions), bits(b.actions))  # the seats swapped: another match
    ended_early = 0
    for r in (a, b):
        for j in range(r.rows):
            gm = r.game(j)
            L = gm["length"]
            assert 1 <= L <= LIMIT and L == int(r.lengths[j])
            assert gm["actions"].shape == (L, 2, 2) and gm["rewards"].shape == (L, 2)
            start = {name: gm["states"][name][0] for name, _, _ in PLANES}
            tr = g.trace_game(start, gm["actions"])
            for name, _, _ in PLANES:
                assert tr[name].shape[0] == L, (j, name)
                assert torch.equal(bits(tr[name]), bits(gm["states"][name][1:])), (j, name)
            misc = gm["states"]["misc"]
            assert misc[:, 0].tolist() == list(range(L + 1))  # the ticks count up from the reset
            live = (misc[:, 1] >> 16) & 0xFF
            assert bool((live[:-1] != 0).all()) and (int(live[-1]) == 0 or L == LIMIT)
            ended_early += L < LIMIT
            # past the row's slabs nothing was written
            for name, _, _ in PLANES:
                assert int(bits(r.states[name][L + 1:, j]).sum()) == 0
            assert int(bits(r.actions[L:, :, j]).sum()) == 0 and int(bits(r.rewards[L:, :, j]).sum()) == 0
    assert ended_early >= 2  # not every recorded game is a draw


def test_recorded_rewards_sum_to_the_returns(played):
    """rewards summed in fp32 in tick order are the leg's per-game returns: a
    per-tick loop driven here over the same games gives them"""
    L, opp = played["L"], played["opp"]
    a = played["res"]["records"][0]
    g = ssa.VecSkillshotGame(GAMES, device="cpu", seed=L._eval_env(GAMES, LIMIT, None).seed, tick_limit=LIMIT)
    g.step_counter = 0
    g.reset(random_positions=True)
    for name, _, _ in PLANES:
        assert torch.equal(bits(getattr(g, name)[:REC]), bits(a.states[name][0])), name
    obs, _ = g.observe()
    alive = torch.ones(GAMES, dtype=torch.bool)
    acc = torch.zeros(2, GAMES)
    with torch.no_grad():
        while bool(alive.any()):
            out = g.step(torch.stack((L.model_actor(obs[0]), opp(obs[1]))), auto_reset=False)
            acc = torch.where(alive[None], acc + out["reward"], acc)
            alive &= ~out["done"].bool()
            obs = out["obs"]
    for j in range(REC):
        s = torch.zeros(2)
        for r in a.game(j)["rewards"]:
            s = s + r
        assert torch.equal(bits(s), bits(acc[:, j])), j
    leg = played["res"]["legs"][0]
    assert leg["mean_return"] == float(acc[0].sum().double()) / GAMES


def test_boards_are_the_reference_painter(played):
    a = played["res"]["records"][0]
    painted = 0
    for j in range(a.rows):
        boards = a.boards(j)
        gm = a.game(j)
        assert boards.dtype == torch.uint8 and boards.shape == (gm["length"] + 1, 250, 250)
        st = gm["states"]
        for s in range(gm["length"] + 1):
            pos, qpos, rot = st["pos"][s].tolist(), st["qpos"][s].tolist(), st["rot"][s].tolist()
            flags = int(st["misc"][s, 1]) & 0xFFFFFFFF
            want = rasterize_board(np.zeros((250, 250), dtype=np.int64), [pos[0:2], pos[2:4]], rot,
                                   [qpos[0:2], qpos[2:4]], [flags & 0xFF, (flags >> 8) & 0xFF])
            assert np.array_equal(boards[s].numpy().astype(np.int64), want), (j, s)
            painted += 1
    assert painted > a.rows * 2


# ---------------------------------------------------------------- league
def test_league_record_rows_are_evaluates_legs(played):
    """league(record=1) with three actors: the row of pairing (i, j) is row 0
    of the evaluate leg that league says it replays (i in seat 1 against j)"""
    L = played["L"]
    B, C = turning_actor(12), turning_actor(13)
    plain = L.league([None, B, C], games=GAMES, tick_limit=LIMIT)
    res = L.league([None, B, C], games=GAMES, tick_limit=LIMIT, record=1)
    rec = res.pop("record")
    assert res == plain
    assert rec.pairs == [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)] and rec.rows == 6 and rec.per_block == 1
    assert rec.games.tolist() == [0] * 6
    legs = {}
    for k, opp in ((1, B), (2, C)):
        e = L.evaluate(opponent=opp, games=GAMES, tick_limit=LIMIT, record=1)["records"]
        legs[(0, k)], legs[(k, 0)] = e  # leg 1: the learner in seat 1; leg 2: the opponent there
    for row, pr in enumerate(rec.pairs):
        if pr not in legs:
            continue
        got, want = rec.game(row), legs[pr].game(0)
        assert got["length"] == want["length"]
        for name, _, _ in PLANES:
            assert torch.equal(bits(got["states"][name]), bits(want["states"][name])), (pr, name)
        assert torch.equal(bits(got["actions"]), bits(want["actions"])), pr
        assert torch.equal(bits(got["rewards"]), bits(want["rewards"])), pr
    lengths = {pr: int(rec.lengths[row]) for row, pr in enumerate(rec.pairs)}
    assert len(legs) == 4 and all(v >= 1 for v in lengths.values())


# ---------------------------------------------------------------- persistence
def test_record_round_trips_through_persist(played, tmp_path):
    a = played["res"]["records"][1]
    path = persist.save_match_record(tmp_path / "records" / "leg2", a)
    assert path.endswith("leg2.npz")
    with np.load(path) as d:
        assert all(d[k].dtype != object for k in d.files)  # arrays and settings only
    b = persist.load_match_record(path)
    for name, _, _ in PLANES:
        assert torch.equal(bits(a.states[name]), bits(b.states[name])) and a.states[name].dtype == b.states[name].dtype
    for f in ("actions", "rewards", "lengths", "games"):
        assert torch.equal(bits(getattr(a, f)), bits(getattr(b, f))) and getattr(a, f).dtype == getattr(b, f).dtype
    assert bytes(a.config) == bytes(b.config) and (b.pairs, b.per_block, b.ticks_run) == (None, a.per_block, a.ticks_run)
    assert torch.equal(a.boards(2), b.boards(2))
    lg = played["L"].league([None, played["opp"]], games=GAMES, tick_limit=LIMIT, record=2)["record"]
    back = persist.load_match_record(persist.save_match_record(str(tmp_path / "league.npz"), lg))
    assert back.pairs == lg.pairs == [(0, 1), (0, 1), (1, 0), (1, 0)] and back.games.tolist() == [0, 1, 0, 1]
    assert torch.equal(bits(back.actions), bits(lg.actions))


def test_board_sequences_play_in_the_replay_format(played, tmp_path):
    """board_sequences() is what save_training_boards takes: it comes back
    from load_training_boards as it went"""
    a = played["res"]["records"][0]
    seqs = a.board_sequences()
    assert len(seqs) == a.rows
    for j, s in enumerate(seqs):
        assert s.dtype == np.int8 and s.shape == (int(a.lengths[j]), 250, 250)
        assert np.array_equal(s, a.boards(j)[1:].numpy().astype(np.int8))
    with_start = a.board_sequences(include_start=True)
    assert all(w.shape[0] == s.shape[0] + 1 and np.array_equal(w[1:], s) for w, s in zip(with_start, seqs))
    L = played["L"]
    old = L.save_location
    try:
        L.save_location = str(tmp_path / "training_models")
        L.save_training_boards(seqs)
        back = L.load_training_boards()
    finally:
        L.save_location = old
    assert len(back) == len(seqs) and all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(back, seqs))
