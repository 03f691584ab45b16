"""k_step_multi's packed instantiation (SK_MULTI_SPLIT=0 with SK_MULTI_PACK=1:
one lane per game, the 48-B resident form between the ticks of a launch)
with restarts in nearly every tick: the packed state goes out right after the
tick and a restarted game's lane stores it again.  Bit for bit one
sk_env_step launch per tick, for both state ports and workgroup sizes and a
partly filled last wave.
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


@pytest.mark.parametrize("block", ["64", "256"])
@pytest.mark.parametrize("pol", [0, 1], ids=["plain", "write_through"])
@pytest.mark.parametrize("n", [33, 3000])
def test_lane_packed_restarts_equal_stepwise(ssa, monkeypatch, pol, n, block):
    monkeypatch.setenv("SK_MULTI_SPLIT", "0")
    monkeypatch.setenv("SK_MULTI_PACK", "1")
    monkeypatch.setenv("SK_MULTI_POLICY", str(pol))
    monkeypatch.setenv("SK_MULTI_BLOCK", block)
    T, R, slab0 = 300, 7, 3
    a = ssa.VecSkillshotGame(n, seed=21, tick_limit=120)
    a.reset(random_positions=True)
    b = ssa.VecSkillshotGame(n, seed=21, tick_limit=120)
    b.load_state_dict(a.state_dict())
    b.step_counter = a.step_counter
    acts = a.gen_random_actions(R)
    a.clear_counters()
    b.clear_counters()
    done, win = a.step_multi(acts, n_ticks=T, slab0=slab0, record=True)
    wd, ww = [], []
    for t in range(T):
        o = b.step(acts[(slab0 + t) % R], obs=False, auto_reset=True)
        wd.append(o["done"].clone())
        ww.append(o["winner"].clone())
    torch.cuda.synchronize()
    assert torch.equal(done, torch.stack(wd))
    assert torch.equal(win, torch.stack(ww))
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert np.array_equal(np.asarray(sa[k]), np.asarray(sb[k])), k
    ca, cb = a.counters(), b.counters()
    assert ca == cb and ca["dones"] > n
