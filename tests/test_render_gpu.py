"""The batched board rasteriser on the GPU (csrc/sk_render.hip): the
reference's boards and the clipped edge set of test_render_cpu.py, the CPU
backend on a thousand played states, a small odd board, a rendered trace, and
model_train's board replay on the on-device episode path.  Every comparison
is exact.  No test gives the device path an out-of-range id."""
import numpy as np
import pytest
import torch

import render_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ssa():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import skillshot_learning_amd as m
    m.load_library()
    return m


@pytest.fixture(scope="module")
def cases(ssa):
    """the fixtures and the edge set in one env, and their expected boards on the device"""
    planes, boards = rc.default_cases()
    g = ssa.VecSkillshotGame(planes["pos"].shape[0], device="cuda")
    g.load_state_dict(planes)
    return g, torch.from_numpy(boards).cuda()


def _render_into_guarded(g, ids, cells):
    """render(ids) into a 16-byte-aligned slice of a larger buffer: 0xAB
    around it, 0xFF inside.  Returns (boards, the bytes before, the bytes after)."""
    m = len(ids)
    lead, tail = 48, 80
    buf = torch.full((lead + m * cells + tail,), 0xAB, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    inside = buf[lead:lead + m * cells]
    inside.fill_(0xFF)
    out = inside.view(m, g.config.board_w, g.config.board_h)
    got = g.render(torch.as_tensor(ids, dtype=torch.int64, device="cuda"), out=out)
    assert got.data_ptr() == out.data_ptr()
    return out, buf[:lead], buf[lead + m * cells:]


@pytest.mark.parametrize("m", [1, 3, 5, 64])
def test_fixtures_and_edge_set_exact(cases, m):
    """M boards per launch at every board-base residue the size allows
    (62,500 % 16 = 4); windows of M ids walk over every state"""
    g, boards = cases
    k = g.n
    for start in range(0, k, m):
        ids = [(start + i) % k for i in range(m)]
        out, before, after = _render_into_guarded(g, ids, 62500)
        assert bool((before == 0xAB).all()) and bool((after == 0xAB).all()), (start, "guard bytes written")
        assert int(out.max()) <= 4, (start, "a byte was not written")
        assert torch.equal(out, boards[ids]), start
    assert torch.equal(g.render(), boards)


def test_gpu_equals_cpu_backend_on_played_states(ssa):
    n = 1021
    g = ssa.VecSkillshotGame(n, device="cuda", seed=1234, tick_limit=2000)
    g.reset(random_positions=True)
    g.rollout_random(300)
    st = g.state_dict()
    c = ssa.VecSkillshotGame(n, device="cpu", seed=1234)
    c.load_state_dict(st)
    want = c.render().cuda()
    assert int((want == 3).sum()) > n and int((want == 4).sum()) > n  # pointers and projectiles are on the boards
    assert torch.equal(g.render(), want)
    ids = torch.randperm(n, generator=torch.Generator().manual_seed(5)).cuda()
    assert torch.equal(g.render(ids), want[ids])


def test_small_odd_board_equals_cpu_backend(ssa):
    from skillshot_learning_amd import _capi
    planes, boards = rc.small_cases()
    cfg = rc.small_config(_capi)
    g = ssa.VecSkillshotGame(5, device="cuda", config=cfg)
    c = ssa.VecSkillshotGame(5, device="cpu", config=cfg)
    g.load_state_dict(planes)
    c.load_state_dict(planes)
    out, before, after = _render_into_guarded(g, list(range(5)), 41 * 23)
    assert bool((before == 0xAB).all()) and bool((after == 0xAB).all())
    assert torch.equal(out.cpu(), c.render())
    assert np.array_equal(out.cpu().numpy(), boards)
    assert torch.equal(g.render([4, 4, 1, 0, 2, 3, 1]).cpu(), c.render([4, 4, 1, 0, 2, 3, 1]))


def test_render_states_of_a_trace(ssa):
    """render_states of one game's 50 recorded states = render after each eager tick"""
    names = [name for name, _, _ in ssa.vec_env.PLANES]
    g = ssa.VecSkillshotGame(8, device="cuda", seed=21, tick_limit=2000)
    g.reset(random_positions=True)
    k = 5
    rec, each = {n_: [] for n_ in names}, []
    for _ in range(50):
        g.step(g.gen_random_actions(1)[0], obs=False, auto_reset=False)
        for n_ in names:
            rec[n_].append(getattr(g, n_)[k].clone())
        each.append(g.render([k])[0])
    got = g.render_states({n_: torch.stack(rec[n_]) for n_ in names})
    assert tuple(got.shape) == (50, 250, 250) and torch.equal(got, torch.stack(each))
    assert len({e.cpu().numpy().tobytes() for e in each}) > 10  # the game moved


@pytest.mark.parametrize("chunk", ["", "7"])
def test_model_train_boards_on_device_equal_loop(ssa, monkeypatch, chunk):
    """model_train(save_boards=True) on the fp32 on-device episode path
    (SK_EPISODE_KERNEL=1: act_episode launches, no get_board) and on the
    per-tick loop (=0): the same board sequences, nets, ticks and winners.
    36 games = two 16-game workgroups and a 4-game one; chunk "7": the
    episodes in launches of 7 ticks."""
    from skillshot_learning_amd import learner, vec_env
    monkeypatch.setenv("SK_FWD16", "0")
    if chunk:
        monkeypatch.setenv("SK_EPISODE_CHUNK", chunk)
    else:
        monkeypatch.delenv("SK_EPISODE_CHUNK", raising=False)
    calls = {"act_episode": 0, "get_board": 0}
    for name in calls:
        orig = getattr(vec_env.VecSkillshotGame, name)

        def spy(self, *a, _orig=orig, _name=name, **kw):
            calls[_name] += 1
            return _orig(self, *a, **kw)
        monkeypatch.setattr(vec_env.VecSkillshotGame, name, spy)
    game, runs = 33, []
    for flag in ("1", "0"):
        monkeypatch.setenv("SK_EPISODE_KERNEL", flag)
        calls.update(act_episode=0, get_board=0)
        L = learner.SkillshotLearner(n_envs=36, device="cuda", seed=9, tick_limit=40, precision="fp32")
        saved = []
        monkeypatch.setattr(L, "save_training_boards", lambda seqs: saved.append(list(seqs)))
        prog = L.model_train(2, save_boards=True, board_game=game)
        torch.cuda.synchronize()
        if flag == "1":
            assert calls["act_episode"] >= 2 and calls["get_board"] == 0, calls
            final = L.game_environment.get_board(game)  # after the spy count: the host painter of the final state
        else:
            assert calls["act_episode"] == 0 and calls["get_board"] > 0, calls
        assert len(saved) == 1 and len(saved[0]) == 2
        runs.append((saved[0], torch.cat([p.detach().flatten() for p in L.model_actor.parameters()]),
                     torch.cat([p.detach().flatten() for p in L.model_critic.parameters()]),
                     torch.stack(prog["epoch_ticks"]), torch.stack(prog["epoch_winner"])))
    (b1, *rest1), (b0, *rest0) = runs
    for x, y in zip(rest1, rest0):
        assert torch.equal(x, y)
    for e in range(2):
        assert b1[e].dtype == np.int8 and b1[e].shape == (int(rest1[2][e][game]), 250, 250)
        assert np.array_equal(b1[e], b0[e]), e
    assert np.array_equal(b1[1][-1], final)
