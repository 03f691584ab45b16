"""Every step kernel at sk_config values other than the reference's (tests/
config_cases.py) against the C oracle, which tests/golden/cfg_*.npz pin to the
reference at these very configurations: the three one-tick kernels, the
multi-tick step under its default plan and forced to the packed split
instantiation (both workgroup sizes, the fp64 carry and the fp32-trig tick,
launches of 1, 7 and 60 ticks), the full-contract multi-tick step with both
rewards, and the register-resident random rollout.  33 and 97 games (a partial
wave; a full wave and a partial one, two workgroups of 64 lanes in the split
geometry), 300 ticks under tick limit 40 with random auto-reset, so every
launch of 60 ticks restarts games inside it (test_config_cpu.py asserts what
the oracle's run contains).

At cfg_wide, cfg_cd128 and cfg_huge the packed kernel's admission refuses the
configuration and the forced launch runs the generic tick; at cfg_look08 and
cfg_look3 a fired projectile's step must not come from sktrig::sincos_add
(look_speed > pi/4), forced fp32-trig tick or not: the results still equal
the oracle's.

Bar: state, done, winner, counters and the RNG step counter bit for bit; obs /
reward / obs_reset within 1e-5 relative to max(1, |ref|); obs[11] exact except
flags that the correctly rounded tan explains one by one (their count is
printed).
"""
import numpy as np
import pytest
import torch

import config_cases as cc
from multi_split_cases import _env
from test_config_cpu import check_limits, check_resets, per_method_ops

pytestmark = pytest.mark.gpu

T = 300
SIZES = [33, 97]


@pytest.fixture(scope="module")
def ssa():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import skillshot_learning_amd as m
    m.load_library()
    return m


@pytest.mark.parametrize("variant", [0, 1, 2], ids=["lane_per_env", "player_split", "fp32_fast"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", cc.NAMES)
def test_step_equals_oracle(ssa, monkeypatch, name, n, variant):
    monkeypatch.setenv("SK_STEP_VARIANT", str(variant))
    cc.play(ssa, "step", name, n, T)


@pytest.mark.parametrize("name", cc.NAMES)
def test_step_simple_reward_equals_oracle(ssa, name):
    cc.play(ssa, "step", name, 97, T, reward="simple")


@pytest.mark.parametrize("launch", [7, 60])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", cc.NAMES)
def test_step_multi_default_plan_equals_oracle(ssa, name, n, launch):
    cc.play(ssa, "multi", name, n, T, launch=launch)


@pytest.mark.parametrize("launch", [1, 7, 60])
@pytest.mark.parametrize("fast", ["0", "1"], ids=["fp64carry", "fast"])
@pytest.mark.parametrize("block", ["64", "512"], ids=["block64", "block512"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", cc.NAMES)
def test_step_multi_packed_split_equals_oracle(ssa, monkeypatch, name, n, block, fast, launch):
    _env(monkeypatch, 0, block, fast)  # the plain port
    cc.play(ssa, "multi", name, n, T, launch=launch)


@pytest.mark.parametrize("name", ["cfg_packed", "cfg_look3"])
def test_step_multi_packed_split_write_through_equals_oracle(ssa, monkeypatch, name):
    _env(monkeypatch, 1, "64", "1")
    cc.play(ssa, "multi", name, 97, T, launch=60)


@pytest.mark.parametrize("reward", ["looking", "simple"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", cc.NAMES)
def test_step_multi_obs_equals_oracle(ssa, name, n, reward):
    cc.play(ssa, "multi_obs", name, n, T, launch=60, reward=reward)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", cc.NAMES)
def test_rollout_random_equals_oracle(ssa, oracle_mod, name, n):
    """sk_env_rollout_random (the fp32-trig tick in registers, random restarts) against the oracle's rollout
    from the cases' start state, in launches of 1, 100 and 199 ticks"""
    tr = cc.oracle_trace(name, n, T)
    ref = oracle_mod.OracleState(n, seed=tr.seed, config=tr.cfg)
    ref.load(tr.start)
    ref.step_counter = tr.step0
    g = cc._engine(ssa, tr, "cuda")
    for chunk in (1, 100, 199):
        g.rollout_random(chunk)
        ref.rollout_random(chunk, tick_limit=cc.TICK_LIMIT)
        torch.cuda.synchronize()
        st = g.state_dict()
        assert st.pop("step_counter") == ref.step_counter
        cc.assert_state_equal(st, ref.arrays(), f"{name} rollout +{chunk}")
    c = g.counters()
    assert [c["dones"], c["hits_p1"], c["hits_p2"], c["ticks_sum"]] == [int(x) for x in ref.counters]
    # the same games as the stepped run: same start, same draws
    cc.assert_state_equal(ref.arrays(), tr.state[T - 1], f"{name} rollout vs steps")
    assert [int(x) for x in ref.counters] == tr.counters


@pytest.mark.parametrize("name", cc.NAMES)
def test_features_equal_oracle(ssa, oracle_mod, name):
    """get_state's numerics (fp64 on the device) on states of the run, at test_gpu_parity.
    test_features_match_oracle's bar: the exact columns equal, the rest within 1e-12"""
    n = 97
    tr = cc.oracle_trace(name, n, T)
    exact = [1, 4, 5, 6, 7, 9, 11, 12, 13, 14, 15, 17]
    for t in (0, 20, T - 1):
        ref = oracle_mod.OracleState(n, config=tr.cfg)
        ref.load(tr.raw[t])
        g = ssa.VecSkillshotGame(n, config=cc.sk_config(name))
        g.load_state_dict(tr.raw[t])
        f, w = g.features().cpu().numpy(), ref.features()
        assert np.array_equal(f[..., exact], w[..., exact]), (name, t)
        assert (np.abs(f - w) <= 1e-12 * np.maximum(1.0, np.abs(w))).all(), (name, t)


def test_per_method_ops_at_cfg_packed(ssa, oracle_mod):
    n = 5000
    per_method_ops(lambda **kw: ssa.VecSkillshotGame(n, **kw), oracle_mod, "cfg_packed", n, lambda x: x.cuda())


@pytest.mark.parametrize("name", cc.NAMES)
def test_resets_follow_the_config(ssa, name):
    check_resets(lambda n, **kw: ssa.VecSkillshotGame(n, **kw), name)


def test_config_limits(ssa):
    check_limits(lambda cfg: ssa.VecSkillshotGame(3, config=cfg))
