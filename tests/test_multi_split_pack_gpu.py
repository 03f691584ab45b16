"""k_step_split_multi's packed instantiation (SK_MULTI_SPLIT=1 with
SK_MULTI_PACK=1: two lanes per game, the 48-B resident form between the
ticks of a launch) must equal one sk_env_step launch per tick bit for bit —
state planes, every tick's done / winner, the RNG step counter and the
episode counters — for both state ports and both workgroup sizes: with
restarts (the early packed store and its re-store), across launch boundaries
(the exchange format), for waves that leave the packed form mid-launch or
never enter it, for ragged batches, and against the CPU backend.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ssa():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import skillshot_learning_amd as m
    m.load_library()
    return m


@pytest.fixture(params=["64", "512"], ids=["block64", "block512"])
def block(request):
    return request.param


def _env(monkeypatch, pol, block):
    monkeypatch.setenv("SK_MULTI_SPLIT", "1")
    monkeypatch.setenv("SK_MULTI_PACK", "1")
    monkeypatch.setenv("SK_MULTI_POLICY", str(pol))
    monkeypatch.setenv("SK_MULTI_BLOCK", block)


def _pair(ssa, n, seed, tick_limit):
    a = ssa.VecSkillshotGame(n, seed=seed, tick_limit=tick_limit)
    a.reset(random_positions=True)
    b = ssa.VecSkillshotGame(n, seed=seed, tick_limit=tick_limit)
    b.load_state_dict(a.state_dict())
    b.step_counter = a.step_counter
    return a, b


def _same_state(x, y):
    sx, sy = x.state_dict(), y.state_dict()
    for k in sx:
        assert np.array_equal(np.asarray(sx[k]), np.asarray(sy[k])), k


def _stepwise(b, acts, T, R, slab0=0):
    wd, ww = [], []
    for t in range(T):
        o = b.step(acts[(slab0 + t) % R], obs=False, auto_reset=True)
        wd.append(o["done"].clone())
        ww.append(o["winner"].clone())
    return torch.stack(wd), torch.stack(ww)


@pytest.mark.parametrize("pol", [0, 1], ids=["plain", "write_through"])
@pytest.mark.parametrize("n", [33, 3000])
def test_restarts_equal_stepwise(ssa, monkeypatch, pol, n, block):
    """Tick limit 120 over 300 ticks: every game restarts several times (the
    early packed store, then the restarted lanes' re-store); the last wave is
    partly filled."""
    _env(monkeypatch, pol, block)
    T, R, slab0 = 300, 7, 3
    a, b = _pair(ssa, n, 21, 120)
    acts = a.gen_random_actions(R)
    a.clear_counters()
    b.clear_counters()
    done, win = a.step_multi(acts, n_ticks=T, slab0=slab0, record=True)
    wd, ww = _stepwise(b, acts, T, R, slab0)
    torch.cuda.synchronize()
    assert torch.equal(done, wd)
    assert torch.equal(win, ww)
    _same_state(a, b)
    assert a.step_counter == b.step_counter
    ca, cb = a.counters(), b.counters()
    assert ca == cb and ca["dones"] > n


@pytest.mark.parametrize("pol", [0, 1], ids=["plain", "write_through"])
def test_launch_lengths_and_last_row(ssa, monkeypatch, pol, block):
    """Launches of 1 (never packed), 13 and 40 ticks, slab0 carried over the
    ring, equal one launch of 54 and 54 single ticks: the exchange format at
    every launch boundary; out_stride 0 leaves the last tick's row."""
    _env(monkeypatch, pol, block)
    n, R = 5000, 11
    a, b = _pair(ssa, n, 4, 2000)
    c = ssa.VecSkillshotGame(n, seed=4, tick_limit=2000)
    c.load_state_dict(a.state_dict())
    c.step_counter = a.step_counter
    acts = a.gen_random_actions(R)
    for g in (a, b, c):
        g.clear_counters()
    s = 0
    for T in (1, 13, 40):
        d_last, w_last = a.step_multi(acts, n_ticks=T, slab0=s)
        s = (s + T) % R
    d_all, w_all = b.step_multi(acts, n_ticks=54, slab0=0, record=True)
    wd, ww = _stepwise(c, acts, 54, R)
    torch.cuda.synchronize()
    assert torch.equal(d_all, wd) and torch.equal(w_all, ww)
    assert torch.equal(d_last, wd[-1]) and torch.equal(w_last, ww[-1])
    _same_state(a, c)
    _same_state(b, c)
    assert a.step_counter == b.step_counter == c.step_counter
    assert a.counters() == b.counters() == c.counters()


@pytest.mark.parametrize("pol", [0, 1], ids=["plain", "write_through"])
def test_waves_leaving_and_never_entering_the_packed_form(ssa, monkeypatch, pol, block):
    """Games whose ticks pass 65,535 in the launch's sixth tick take their
    waves out of the packed form mid-launch; a game with only player 2's
    cooldown at -900 keeps its wave in the 88-B form for the whole launch
    while its neighbours pack."""
    _env(monkeypatch, pol, block)
    n, T, R = 3000, 20, 3
    a, b = _pair(ssa, n, 33, 10 ** 6)
    st = a.state_dict()
    st["misc"][[5, 700, 701, 2999], 0] = 65530
    st["qcdage"][[130, 1500], 2] = -900
    for g in (a, b):
        g.load_state_dict(st)
        g.clear_counters()
    acts = a.gen_random_actions(R)
    done, win = a.step_multi(acts, n_ticks=T, record=True)
    wd, ww = _stepwise(b, acts, T, R)
    torch.cuda.synchronize()
    assert torch.equal(done, wd) and torch.equal(win, ww)
    _same_state(a, b)
    assert a.step_counter == b.step_counter
    assert a.counters() == b.counters()


def test_cpu_backend_equals_gpu(ssa, monkeypatch, block):
    _env(monkeypatch, 1, block)
    n, T, R = 4096, 260, 5
    g = ssa.VecSkillshotGame(n, seed=9, tick_limit=100)
    g.reset(random_positions=True)
    c = ssa.VecSkillshotGame(n, device="cpu", seed=9, tick_limit=100)
    c.load_state_dict(g.state_dict())
    acts = g.gen_random_actions(R)
    g.clear_counters()
    c.clear_counters()
    dg, wg = g.step_multi(acts, n_ticks=T, slab0=2, record=True)
    dc, wc = c.step_multi(acts.cpu(), n_ticks=T, slab0=2, record=True)
    assert np.array_equal(dg.cpu().numpy(), dc.numpy())
    assert np.array_equal(wg.cpu().numpy(), wc.numpy())
    _same_state(g, c)
    assert g.counters() == c.counters()


def test_capture_before_the_pack_buffer_exists(ssa, monkeypatch, block):
    """The first multi-tick launch of a small env (no pack buffer yet) is
    captured into a graph: nothing is allocated on the capturing stream, the
    captured launch runs the 88-B form and the replay equals the stepwise
    ticks."""
    import ctypes
    _env(monkeypatch, 1, block)
    n, T, R = 3000, 30, 4
    a, b = _pair(ssa, n, 5, 25)
    acts = a.gen_random_actions(R)
    done = torch.zeros(n, dtype=torch.uint8, device="cuda")
    a.clear_counters()
    b.clear_counters()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        a.step_multi_raw(ctypes.c_void_p(acts.data_ptr()), R, 0, T, ctypes.c_void_p(done.data_ptr()), None, 0,
                         stream=ctypes.c_void_p(st.cuda_stream))
    with torch.cuda.stream(st):
        g.replay()
    st.synchronize()
    wd, _ = _stepwise(b, acts, T, R)
    torch.cuda.synchronize()
    assert torch.equal(done, wd[-1])
    _same_state(a, b)
    assert a.step_counter == b.step_counter
    assert a.counters() == b.counters()


def test_512_lane_geometry_over_many_workgroups(ssa, monkeypatch):
    """40,000 games on 512-lane workgroups: 157 workgroups, the last one
    partly filled (64 of its 256 games)."""
    _env(monkeypatch, 1, "512")
    n, T, R = 40000, 120, 5
    a, b = _pair(ssa, n, 7, 50)
    acts = a.gen_random_actions(R)
    a.clear_counters()
    b.clear_counters()
    done, win = a.step_multi(acts, n_ticks=T, slab0=1, record=True)
    wd, ww = _stepwise(b, acts, T, R, 1)
    torch.cuda.synchronize()
    assert torch.equal(done, wd) and torch.equal(win, ww)
    _same_state(a, b)
    assert a.step_counter == b.step_counter
    ca, cb = a.counters(), b.counters()
    assert ca == cb and ca["dones"] > n
