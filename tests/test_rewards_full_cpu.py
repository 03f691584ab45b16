"""F3: calculate_rewards (SkillshotLearner.py:605-661), the episode-level
reward with credit assignment at the winner's firing tick, batched in torch.

Pinned against the reference itself: make_golden.py runs the reference's
calculate_rewards over each learner-protocol episode's get_state() list and
stores `reward_full` (all-NaN for an episode on which it raises IndexError).
The reward is checked bit-exactly on the reference's own per-tick
projectile_dist_opponent (`reward_full_dist`), with the future-collision flag
and projectile age from the C oracle's get_state() numerics on the fixture's
states.  Those distances depend on the coordinates' Python types in the
reference (SkillshotGame.py:133-134: Python-int `x ** 0.5` is libm pow, which
is not always the correctly rounded sqrt -- pow(19125, .5) is 1 ulp above it;
np.int64 positions of the random start take numpy's exact sqrt), so they are
checked separately against the oracle to 1 ulp."""
import numpy as np
import pytest
import torch

from golden_replay import config_of, fixture_names, load, max_dist_of, state_at
from skillshot_learning_amd.learner import calculate_rewards_full

FULL = [n for n in fixture_names() if "reward_full" in np.load(f"tests/golden/{n}.npz").files]


def _inputs(oracle_mod, d):
    E = d["pos"].shape[0]
    T = int(d["n_steps"].max())
    feats = []
    for t in range(1, T + 1):
        st = oracle_mod.OracleState(E, config=config_of(d))
        st.load(state_at(d, t))
        feats.append(st.features())
    f = torch.from_numpy(np.stack(feats))                       # [T, E, 2, 18]
    want = d["reward_full_dist"][:, :T]                         # [E, T, 2]
    got = f[..., 16].permute(1, 0, 2).numpy()
    m = ~np.isnan(want)
    assert (np.abs(got[m] - want[m]) <= np.spacing(want[m])).all()
    dist = torch.from_numpy(np.ascontiguousarray(np.nan_to_num(want).transpose(1, 0, 2)))
    winner = torch.from_numpy(d["winner"][:, 1:T + 1].T.astype(np.int64))
    return dist, f[..., 17] != 0, f[..., 14].long(), winner, torch.from_numpy(d["n_steps"].astype(np.int64))


def test_full_reward_fixtures_present():
    assert len(FULL) >= 6


@pytest.mark.parametrize("name", FULL)
def test_calculate_rewards_full_matches_reference(oracle_mod, name):
    d = load(name)
    dist, fc, age, winner, lengths = _inputs(oracle_mod, d)
    r, raised = calculate_rewards_full(dist, fc, age, winner, lengths, max_dist=max_dist_of(config_of(d)))
    want = d["reward_full"]                                     # [E, T, 2]
    want_raised = np.isnan(want[:, 0, 0])
    assert np.array_equal(raised.numpy(), want_raised)
    got = r.permute(1, 0, 2).numpy()
    for e in range(want.shape[0]):
        if want_raised[e]:
            continue
        n = int(d["n_steps"][e])
        assert np.array_equal(got[e, :n], want[e, :n]), (name, e, np.argwhere(got[e, :n] != want[e, :n])[:3])
        assert np.isnan(got[e, n:]).all()


def test_calculate_rewards_full_quirks():
    """Hand cases: multipliers, negative-index wrap, IndexError games."""
    T, N = 4, 4
    dist = torch.tensor([[10.0, 20.0]]).expand(T, N, 2).clone()
    fc = torch.zeros(T, N, 2, dtype=torch.bool)
    fc[0, 0, 0] = True
    age = torch.zeros(T, N, 2, dtype=torch.long)
    winner = torch.zeros(T, N, dtype=torch.long)
    winner[3, 1], age[3, 1, 1] = 2, 1       # fired at tick 2
    winner[3, 2], age[3, 2, 0] = 1, 5       # 3 - 5 = -2 -> wraps to tick 1
    winner[3, 3], age[3, 3, 0] = 1, 7       # 3 - 7 = -4 -> IndexError
    r, raised = calculate_rewards_full(dist, fc, age, winner, max_dist=1.0)
    assert raised.tolist() == [False, False, False, True]
    assert r[0, 0].tolist() == [20 - 10 * 0.5, 10 - 20 * 0.75]
    assert r[1, 0].tolist() == [20 - 10 * 0.75, 10 - 20 * 0.75]
    assert r[2, 1, 1] == 1 and r[3, 1].tolist() == [20 - 10 * 2.75, 10 - 20 * 0.75]
    assert r[1, 2, 0] == 1 and r[3, 2].tolist() == [20 - 10 * 0.75, 10 - 20 * 2.75]
    assert torch.isnan(r[:, 3]).all()
    # age 0 at a won tick indexes the tick itself: out of range -> raises
    age2 = torch.zeros(T, 1, 2, dtype=torch.long)
    w2 = torch.zeros(T, 1, dtype=torch.long)
    w2[2, 0] = 1
    _, raised2 = calculate_rewards_full(dist[:, :1], fc[:, :1], age2, w2)
    assert raised2.tolist() == [True]
