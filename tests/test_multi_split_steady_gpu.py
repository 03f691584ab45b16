"""The packed split kernel's peeled launch (k_step_split_multi, PACK: tick 0
and the last tick on the generic tick, the steady loop between them) must
equal one sk_env_step launch per tick bit for bit: state planes, every
tick's done / winner row, the RNG step counter and the episode counters.
The path is forced with SK_MULTI_SPLIT=1 and SK_MULTI_PACK=1, for both trig
forms (SK_MULTI_FAST 0 / 1), both state ports and both workgroup sizes.
"""
import ctypes

import numpy as np
import pytest
import torch

from multi_split_cases import _env, block, fast, pol  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ssa():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import skillshot_learning_amd as m
    m.load_library()
    return m


def _pair(ssa, n, seed, tick_limit, random_positions=True):
    a = ssa.VecSkillshotGame(n, seed=seed, tick_limit=tick_limit, random_positions=random_positions)
    a.reset(random_positions=True)
    b = ssa.VecSkillshotGame(n, seed=seed, tick_limit=tick_limit, random_positions=random_positions)
    b.load_state_dict(a.state_dict())
    b.step_counter = a.step_counter
    return a, b


def _same_state(x, y):
    sx, sy = x.state_dict(), y.state_dict()
    for k in sx:
        assert np.array_equal(np.asarray(sx[k]), np.asarray(sy[k])), k


def _stepwise(b, acts, T, R, slab0=0, auto_reset=True):
    wd, ww = [], []
    for t in range(T):
        o = b.step(acts[(slab0 + t) % R], obs=False, auto_reset=auto_reset)
        wd.append(o["done"].clone())
        ww.append(o["winner"].clone())
    return torch.stack(wd), torch.stack(ww)


def _same_rest(a, b):
    _same_state(a, b)
    assert a.step_counter == b.step_counter
    assert a.counters() == b.counters()


@pytest.mark.parametrize("record", [True, False], ids=["record", "last_row"])
def test_launch_lengths_over_a_wrapping_ring(ssa, monkeypatch, pol, block, fast, record):
    """1, 2, 3, 4, 5 and 9 ticks per launch on a ring of 3 slabs from slab 2:
    first == last tick, no steady tick, exactly one, odd and even counts for
    the alternating action registers; the ring wraps inside the steady loop.
    Every row recorded, and out_stride 0 (the last tick's row only)."""
    _env(monkeypatch, pol, block, fast)
    n, R = 200, 3
    a, b = _pair(ssa, n, 11, 6)
    acts = a.gen_random_actions(R)
    a.clear_counters()
    b.clear_counters()
    s = 2
    for T in (1, 2, 3, 4, 5, 9):
        done, win = a.step_multi(acts, n_ticks=T, slab0=s, record=record)
        wd, ww = _stepwise(b, acts, T, R, s)
        torch.cuda.synchronize()
        if record:
            assert torch.equal(done, wd) and torch.equal(win, ww), T
        else:
            assert torch.equal(done, wd[-1]) and torch.equal(win, ww[-1]), T
        _same_rest(a, b)
        s = (s + T) % R
    assert a.counters()["dones"] > 0


@pytest.mark.parametrize("n", [1, 33])
def test_ragged_batches(ssa, monkeypatch, pol, block, fast, n):
    """A wave with two live lanes, and one with lanes past the batch's end."""
    _env(monkeypatch, pol, block, fast)
    T, R = 23, 4
    a, b = _pair(ssa, n, 3, 5)
    acts = a.gen_random_actions(R)
    a.clear_counters()
    b.clear_counters()
    done, win = a.step_multi(acts, n_ticks=T, slab0=1, record=True)
    wd, ww = _stepwise(b, acts, T, R, 1)
    torch.cuda.synchronize()
    assert torch.equal(done, wd) and torch.equal(win, ww)
    _same_rest(a, b)
    assert a.counters()["dones"] > 0


def test_a_wave_leaves_the_steady_loop_and_comes_back(ssa, monkeypatch, pol, block, fast):
    """Games at 65,530 ticks under a limit of 65,540 stop fitting the packed
    form at the sixth tick of 30, restart a few ticks later and fit again;
    the other waves stay packed throughout; one game in another wave starts
    with player 2's cooldown at -900."""
    _env(monkeypatch, pol, block, fast)
    n, T, R = 200, 30, 3
    a, b = _pair(ssa, n, 33, 65540)
    st = a.state_dict()
    st["misc"][[5, 6, 40], 0] = 65530
    st["qcdage"][[100], 2] = -900
    for g in (a, b):
        g.load_state_dict(st)
        g.clear_counters()
    acts = a.gen_random_actions(R)
    done, win = a.step_multi(acts, n_ticks=T, record=True)
    wd, ww = _stepwise(b, acts, T, R)
    torch.cuda.synchronize()
    assert torch.equal(done, wd) and torch.equal(win, ww)
    _same_rest(a, b)
    assert a.counters()["dones"] >= 3


@pytest.mark.parametrize("mode", ["random", "fixed", "no_reset"])
def test_restarts_inside_the_steady_loop(ssa, monkeypatch, pol, block, fast, mode):
    """Tick limit 7 over 40 ticks: every game finishes inside the steady loop,
    restarting at random or fixed positions, or (auto_reset = 0) staying
    finished, its done flag 1 on every later tick."""
    _env(monkeypatch, pol, block, fast)
    n, T, R = 96, 40, 5
    a, b = _pair(ssa, n, 17, 7, random_positions=(mode != "fixed"))
    acts = a.gen_random_actions(R)
    a.clear_counters()
    b.clear_counters()
    ar = mode != "no_reset"
    done, win = a.step_multi(acts, n_ticks=T, slab0=3, record=True, auto_reset=ar)
    wd, ww = _stepwise(b, acts, T, R, 3, auto_reset=ar)
    torch.cuda.synchronize()
    assert torch.equal(done, wd) and torch.equal(win, ww)
    _same_rest(a, b)
    assert a.counters()["dones"] >= n
    if not ar:
        d = done.cpu().numpy()
        assert d[-1].all() and (d[1:] >= d[:-1]).all()


@pytest.mark.parametrize("outs", ["winner_only", "done_only", "both"])
def test_null_outputs(ssa, monkeypatch, pol, block, fast, outs):
    _env(monkeypatch, pol, block, fast)
    n, T, R = 96, 12, 4
    a, b = _pair(ssa, n, 8, 5)
    acts = a.gen_random_actions(R)
    a.clear_counters()
    b.clear_counters()
    done = torch.full((T, n), 0xAA, dtype=torch.uint8, device="cuda")
    win = torch.full((T, n), 0xAA, dtype=torch.uint8, device="cuda")
    a.step_multi_raw(ctypes.c_void_p(acts.data_ptr()), R, 1, T,
                     ctypes.c_void_p(done.data_ptr()) if outs != "winner_only" else None,
                     ctypes.c_void_p(win.data_ptr()) if outs != "done_only" else None, n)
    wd, ww = _stepwise(b, acts, T, R, 1)
    torch.cuda.synchronize()
    assert torch.equal(done, wd) if outs != "winner_only" else bool((done == 0xAA).all())
    assert torch.equal(win, ww) if outs != "done_only" else bool((win == 0xAA).all())
    _same_rest(a, b)


def test_captured_launch_replayed_twice(ssa, monkeypatch, pol, block, fast):
    """The pack buffer exists before the capture (one eager launch); the graph
    holds the step-slot sync and one 12-tick launch, replayed twice."""
    _env(monkeypatch, pol, block, fast)
    n, T, R = 200, 12, 4
    a, b = _pair(ssa, n, 5, 9)
    acts = a.gen_random_actions(R)
    done = torch.zeros(n, dtype=torch.uint8, device="cuda")
    win = torch.zeros(n, dtype=torch.uint8, device="cuda")
    a.clear_counters()
    b.clear_counters()
    a.step_multi(acts, n_ticks=2, slab0=0)
    _stepwise(b, acts, 2, R, 0)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    s = ctypes.c_void_p(st.cuda_stream)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        a.sync_step_counter(stream=s)
        a.step_multi_raw(ctypes.c_void_p(acts.data_ptr()), R, 2, T, ctypes.c_void_p(done.data_ptr()),
                         ctypes.c_void_p(win.data_ptr()), 0, stream=s)
    with torch.cuda.stream(st):
        g.replay()
        g.replay()
    st.synchronize()
    for _ in range(2):
        wd, ww = _stepwise(b, acts, T, R, 2)
    torch.cuda.synchronize()
    assert torch.equal(done, wd[-1]) and torch.equal(win, ww[-1])
    _same_rest(a, b)
    assert a.counters()["dones"] > 0
