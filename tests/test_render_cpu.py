"""The batched board rasteriser (sk_env_render / sk_render_states,
VecSkillshotGame.render / render_states / trace_game) on libskillshot's CPU
backend: the reference's boards, the clipped edge set, id gathers, the error
and alignment contract, a small odd board, and the trace replay.  Every
comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

import render_cases as rc


@pytest.fixture(scope="module")
def ssa():
    import skillshot_learning_amd as m
    m.load_library()
    return m


@pytest.fixture(scope="module")
def capi():
    from skillshot_learning_amd import _capi
    _capi.load()
    return _capi


@pytest.fixture(scope="module")
def cases():
    return rc.default_cases()


def _env(ssa, planes, **kw):
    g = ssa.VecSkillshotGame(planes["pos"].shape[0], device="cpu", **kw)
    g.load_state_dict(planes)
    return g


def test_render_matches_reference_boards(ssa):
    planes, boards = rc.golden_states()
    got = _env(ssa, planes).render()
    assert got.dtype == torch.uint8 and tuple(got.shape) == boards.shape
    assert np.array_equal(got.numpy(), boards)


def test_render_edge_set_is_the_clipped_painter(ssa, cases):
    planes, boards = cases
    got = _env(ssa, planes).render().numpy()
    for k in range(boards.shape[0]):
        assert np.array_equal(got[k], boards[k]), k
    # the set does exercise what it names: every colour, undrawn pointers, one board with both players off it
    assert (boards.reshape(len(boards), -1).max(1) == 0).sum() == 1 and set(np.unique(boards)) == {0, 1, 2, 3, 4}
    assert any((b == 3).sum() == 0 for b in boards) and any((b == 4).sum() == 0 for b in boards)


def test_render_ids_gather(ssa, cases):
    planes, boards = cases
    g = _env(ssa, planes)
    n = g.n
    ids = [n - 1, 3, 3, 0, n - 2, 3, 1, 0]
    assert np.array_equal(g.render(ids).numpy(), boards[ids])
    assert np.array_equal(g.render(np.array(ids[::-1])).numpy(), boards[ids[::-1]])
    assert np.array_equal(g.render(torch.tensor(ids)).numpy(), boards[ids])
    assert g.render([]).shape == (0, 250, 250)
    out = torch.full((2, 250, 250), 0xFF, dtype=torch.uint8)
    assert g.render([5, 4], out=out) is out and np.array_equal(out.numpy(), boards[[5, 4]])
    for bad in ([0, -1], [n], np.array([1, n, 2])):
        with pytest.raises(IndexError):
            g.render(bad)


def test_raw_abi_out_of_range_id_is_a_zero_board(ssa, capi, cases):
    planes, boards = cases
    g = _env(ssa, planes)
    L = capi.load()
    ids = torch.tensor([2, -1, g.n, 1, 2 ** 40, -2 ** 40], dtype=torch.int64)
    out = torch.full((6, 250, 250), 0xFF, dtype=torch.uint8)
    assert L.sk_env_render(g._h, ids.data_ptr(), 6, out.data_ptr(), None) == capi.SK_OK
    want = np.zeros((6, 250, 250), np.uint8)
    want[0], want[3] = boards[2], boards[1]
    assert np.array_equal(out.numpy(), want)


def test_error_and_alignment_contract(ssa, capi, cases):
    planes, _ = cases
    g = _env(ssa, planes)
    L = capi.load()
    cfg = capi.default_config()
    view = capi.SkStateView(g.n, *[getattr(g, name).data_ptr() for name, _, _ in ssa.vec_env.PLANES])
    buf = torch.zeros(2 * 62500 + 64, dtype=torch.uint8)
    base = buf.data_ptr()
    assert base % 16 == 0
    out = ctypes.c_void_p(base)

    def einval(rc_, word):
        assert rc_ == capi.SK_EINVAL and word in L.sk_last_error().decode(), (rc_, L.sk_last_error())

    einval(L.sk_env_render(None, None, 1, out, None), "NULL")
    einval(L.sk_env_render(g._h, None, 1, None, None), "out")
    einval(L.sk_render_states(ctypes.byref(cfg), -1, None, None, 1, out, None), "view")
    einval(L.sk_render_states(ctypes.byref(cfg), -1, ctypes.byref(view), None, 1, None, None), "out")
    einval(L.sk_env_render(g._h, None, -1, out, None), "m ")
    einval(L.sk_render_states(ctypes.byref(cfg), -1, ctypes.byref(view), None, -3, out, None), "m ")
    # a misaligned out: the slice at byte offset 4
    einval(L.sk_env_render(g._h, None, 1, ctypes.c_void_p(base + 4), None), "aligned")
    einval(L.sk_render_states(ctypes.byref(cfg), -1, ctypes.byref(view), None, 1, ctypes.c_void_p(base + 4), None),
           "aligned")
    with pytest.raises(ssa.SkillshotError, match="aligned"):
        g.render([0, 1], out=buf[4:4 + 2 * 62500].view(2, 250, 250))
    # the sprite images are fixed: other sizes are refused
    for field, value in (("player_size", 4), ("projectile_size", 5)):
        bad = capi.default_config()
        setattr(bad, field, value)
        einval(L.sk_render_states(ctypes.byref(bad), -1, ctypes.byref(view), None, 1, out, None), "sprites")
        gb = ssa.VecSkillshotGame(2, device="cpu", config=bad)
        einval(L.sk_env_render(gb._h, None, 1, out, None), "sprites")
    missing = capi.SkStateView(g.n, g.pos.data_ptr(), None, g.qpos.data_ptr(), g.qrot.data_ptr(),
                               g.qcdage.data_ptr(), g.misc.data_ptr())
    einval(L.sk_render_states(ctypes.byref(cfg), -1, ctypes.byref(missing), None, 1, out, None), "view")
    # m == 0 is a successful no-op
    buf.fill_(0xAB)
    assert L.sk_env_render(g._h, None, 0, out, None) == capi.SK_OK
    assert L.sk_render_states(ctypes.byref(cfg), -1, ctypes.byref(view), None, 0, out, None) == capi.SK_OK
    assert bool((buf == 0xAB).all())
    # NULL cfg = the reference values
    assert L.sk_render_states(None, -1, ctypes.byref(view), None, 2, out, None) == capi.SK_OK
    assert torch.equal(buf[:2 * 62500].view(2, 250, 250), g.render([0, 1]))
    # wrong out tensors are refused before the library sees them
    for bad_out in (torch.zeros((2, 250, 250), dtype=torch.int8), torch.zeros((3, 250, 250), dtype=torch.uint8),
                    torch.zeros((2, 250, 500), dtype=torch.uint8)[:, :, ::2]):
        with pytest.raises(ValueError):
            g.render([0, 1], out=bad_out)


def test_small_odd_board(ssa, capi):
    planes, boards = rc.small_cases()
    g = _env(ssa, planes, config=rc.small_config(capi))
    got = g.render()
    assert tuple(got.shape) == (5, 41, 23)
    assert np.array_equal(got.numpy(), boards)
    assert np.array_equal(g.render([4, 0, 4]).numpy(), boards[[4, 0, 4]])
    assert np.array_equal(g.render_states({k: torch.as_tensor(v) for k, v in planes.items()}).numpy(), boards)


def test_trace_game_replays_a_recorded_episode(ssa):
    """a random-policy episode of one game of a CPU-backend batch, recorded
    tick by tick: trace_game from its start row and actions returns the
    recorded planes exactly and stops where the game ended"""
    names = [name for name, _, _ in ssa.vec_env.PLANES]
    g = ssa.VecSkillshotGame(6, device="cpu", seed=11, tick_limit=300)
    g.reset(random_positions=True)
    k = 4
    start = {n_: getattr(g, n_)[k].clone() for n_ in names}
    acts, rec, end = [], {n_: [] for n_ in names}, None
    for t in range(330):
        a = g.gen_random_actions(1)[0]
        done = g.step(a, obs=False, auto_reset=False)["done"]
        acts.append(a[:, k].clone())
        for n_ in names:
            rec[n_].append(getattr(g, n_)[k].clone())
        if end is None and bool(done[k]):
            end = t + 1
    assert end is not None and 1 < end <= 300
    tr = g.trace_game(start, torch.stack(acts))  # 330 actions: the replay stops at the game's end
    for n_ in names:
        want = torch.stack(rec[n_][:end])
        assert tr[n_].shape == want.shape and tr[n_].dtype == want.dtype
        assert np.array_equal(tr[n_].numpy().view(np.uint8), want.numpy().view(np.uint8)), n_
    short = g.trace_game(start, torch.stack(acts[:5]))  # fewer actions than the episode: every tick of them
    assert short["pos"].shape[0] == 5 and torch.equal(short["misc"], tr["misc"][:5])
    boards = g.render_states(tr)
    assert tuple(boards.shape) == (end, 250, 250)
    last = ssa.VecSkillshotGame(1, device="cpu")
    last.load_state_dict({n_: tr[n_][-1:].numpy() for n_ in names})
    assert np.array_equal(boards[-1].numpy(), last.get_board(0))
