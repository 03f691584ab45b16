"""Shared by tests/test_graph_handover_gpu.py (and its CPU condition check,
tests/test_graph_handover_cpu.py): the CPU-backend twin of a GPU environment,
the comparison bar, and part A's schedule of graph replays and eager calls.

The reference is VecSkillshotGame(device="cpu") (csrc/sk_host.cpp): one host
step counter, no device slots, itself pinned to the C oracle and the golden
fixtures (tests/test_host_backend_cpu.py).  It cannot go wrong the way the
two-slot counter can, whatever the cut of the ticks into graphs.

"Equal": every state plane bit for bit, step_counter, counters().
Observations: within OBS_TOL relative to max(1, |ref|), the future-collision
flag (column 11) exact, as tests/test_gpu_parity.py."""
import numpy as np
import torch

OBS_TOL = 1e-5


def cpu_twin(ssa, g):
    """a CPU-backend environment with g's parameters and current state (its
    step_counter the true one, the slots' maximum); both sides' episode
    counters start from zero"""
    c = ssa.VecSkillshotGame(g.n, device="cpu", seed=g.seed, env_offset=g.env_offset, tick_limit=g.tick_limit,
                             random_positions=g.random_positions, config=g.config)
    c.load_state_dict(g.state_dict())
    g.clear_counters()
    c.clear_counters()
    return c


def assert_equal(g, c, where):
    sg, sc = g.state_dict(), c.state_dict()
    kg, kc = sg.pop("step_counter"), sc.pop("step_counter")
    assert kg == kc, (where, "step_counter", kg, kc)
    for k in sc:
        assert np.array_equal(np.asarray(sg[k]).view(np.uint8), np.asarray(sc[k]).view(np.uint8)), (where, k)
    assert g.counters() == c.counters(), where


def assert_obs(got, want, where, flag=True):
    x = got.detach().cpu().numpy().astype(np.float64)
    y = want.detach().cpu().numpy().astype(np.float64)
    err = (np.abs(x - y) / np.maximum(1.0, np.abs(y))).max()
    assert err <= OBS_TOL, (where, err)
    if flag:
        assert np.array_equal(x[..., 11], y[..., 11]), (where, "flag")


def slabs(seed, k, n):
    """k action slabs [k, 2, n, 2] from a seeded host generator"""
    return torch.from_numpy(np.random.default_rng(seed).uniform(-1.0, 1.0, (k, 2, n, 2)).astype(np.float32))


# ------------------------------------------------------------------ part A
A_N, A_SEED, A_OFFSET, A_LIMIT = 70, 11, 5, 4
# graph name -> (entry point, number of ticks, first slab of A_GRAPH_SLABS)
A_GRAPHS = {"s3": ("step", 3, 0), "s2": ("step", 2, 3), "m5": ("step_multi", 5, 5)}
A_GRAPH_SLABS = 10
# (graphs replayed in order, the eager call after them, its ticks)
A_SCHEDULE = [
    ((), "step", 1),
    (("s3",), "step", 2),
    (("s3", "s3"), "step_multi", 3),
    (("s2", "m5"), "reset", 0),
    (("s3",), "gen_random_actions", 2),
    (("s3",), "rollout_random", 5),
    (("s3",), "step_multi_obs", 3),
]
A_EAGER_SLABS = sum(t for _, _, t in A_SCHEDULE)


def a_env(ssa, device):
    """part A's environment: 70 games (the last workgroup partial), random
    restarts, every game restarts at least every fourth tick; three ticks
    into its episodes, so the schedule's first eager step already restarts"""
    g = ssa.VecSkillshotGame(A_N, device=device, seed=A_SEED, env_offset=A_OFFSET, tick_limit=A_LIMIT,
                             random_positions=True)
    g.reset(random_positions=True)
    g.rollout_random(3)
    return g


def a_mask():
    return (torch.arange(A_N) % 3 == 0).to(torch.uint8)


def a_replay_on(env, name, graph_slabs):
    """what a replay of graph `name` computes, as plain calls on `env`"""
    kind, ticks, s0 = A_GRAPHS[name]
    a = graph_slabs[s0:s0 + ticks].to(env.device)
    if kind == "step":
        for t in range(ticks):
            env.step(a[t], obs=True, auto_reset=True)
    else:
        env.step_multi(a.contiguous(), ticks)


def a_eager_on(env, call, ticks, acts):
    """the schedule's eager call on `env` (either backend) with the action
    slabs `acts` [ticks, 2, n, 2]; returns what the call hands back"""
    a = acts.to(env.device).contiguous()
    if call == "step":
        return [env.step(a[t], obs=True, auto_reset=True) for t in range(ticks)][-1]
    if call == "step_multi":
        return env.step_multi(a, ticks)
    if call == "reset":
        return env.reset(mask=a_mask().to(env.device), random_positions=True)
    if call == "gen_random_actions":
        drawn = env.gen_random_actions(ticks)
        for t in range(ticks):
            env.step(drawn[t], obs=True, auto_reset=True)
        return drawn
    if call == "rollout_random":
        return env.rollout_random(ticks)
    if call == "step_multi_obs":
        return env.step_multi_obs(a, ticks)
    raise ValueError(call)


def a_reference_windows(ssa):
    """the whole schedule on the CPU backend alone: per item, the dones
    counted inside its eager window and the games its eager call moved
    (for the restart condition, which the reference alone must satisfy)"""
    c = a_env(ssa, "cpu")
    c.clear_counters()
    gs, es = slabs(101, A_GRAPH_SLABS, A_N), slabs(202, A_EAGER_SLABS, A_N)
    out, e0 = [], 0
    for graphs, call, ticks in A_SCHEDULE:
        for name in graphs:
            a_replay_on(c, name, gs)
        before, pos = c.counters()["dones"], c.state_dict()["pos"].copy()
        a_eager_on(c, call, ticks, es[e0:e0 + ticks])
        e0 += ticks
        moved = (c.state_dict()["pos"].reshape(A_N, -1) != pos.reshape(A_N, -1)).any(1)
        out.append((call, c.counters()["dones"] - before, moved))
    return out


def assert_a_condition(windows):
    """Every eager window holds restarts (else a stale key changes nothing
    and the comparison is vacuous): dones grow inside each stepping window;
    the reset window draws the keyed random start itself, for every masked
    game."""
    mask = a_mask().numpy().astype(bool)
    for i, (call, dones, moved) in enumerate(windows):
        if call == "reset":
            assert moved[mask].all() and not moved[~mask].any(), i
        else:
            assert dones > 0, (i, call)
