"""bench.py's child-process guard: every one-GPU
secondary leg runs in a child under a timeout, so a hung leg is killed and
reported and the headline line still prints.  CPU only: the guard itself."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_child_results_and_exit_code():
    ok, res, _ = bench._child([sys.executable, "-c", "print('{\"a\": 1}'); print('noise'); print('{\"b\": 2}')"],
                              dict(os.environ), 30, "t")
    assert ok and res == [{"a": 1}, {"b": 2}]
    ok, res, err = bench._child([sys.executable, "-c", "import sys; print('{\"a\": 1}'); sys.exit(3)"],
                                dict(os.environ), 30, "t")
    assert not ok and res == [{"a": 1}]


def test_child_killed_at_timeout_keeps_finished_results():
    t0 = time.time()
    ok, res, err = bench._child([sys.executable, "-c",
                                 "import time; print('{\"first\": 1}', flush=True); time.sleep(120)"],
                                dict(os.environ), 3, "t")
    assert time.time() - t0 < 30
    assert not ok and res == [{"first": 1}] and "killed" in err


def test_plain_and_full_options(monkeypatch):
    """--steps / --warmup are what the timed region uses; --full and
    --dump-outputs are off unless given"""
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (20, 5, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.no_full and a.dump_outputs == "d"


class _FakeEnv:
    """what dump_outputs reads of the env the headline ran on"""

    def __init__(self, n):
        import numpy as np
        import torch
        from types import SimpleNamespace
        self.n = n
        self.bench_stream = SimpleNamespace(cuda_stream=0)
        self.bench_done = torch.arange(n, dtype=torch.uint8) % 2
        self._st = dict(pos=np.arange(4 * n, dtype=np.int32).reshape(n, 4) - 7,
                        rot=np.linspace(-3, 3, 2 * n).reshape(n, 2), step_counter=(1 << 40) + 3)

    def state_dict(self):
        return dict(self._st)

    def counters(self, stream=None):
        return dict(dones=5, hits_p1=1, hits_p2=2, ticks_sum=99)


def test_dump_outputs_formats_and_bounded_sample(tmp_path):
    """float32 / float64 files that hold the values exactly; past the byte
    budget a fixed, sorted sample of the games (the same every time), its ids
    in games.npy, and never more than the budget in all"""
    import numpy as np
    n = 1000
    env = _FakeEnv(n)
    bench.dump_outputs(str(tmp_path / "all"), env)
    got = {f[:-4]: np.load(tmp_path / "all" / f) for f in os.listdir(tmp_path / "all")}
    assert sorted(got) == ["counters", "done", "pos", "rot", "step_counter"]
    assert got["done"].dtype == np.float32 and np.array_equal(got["done"], env.bench_done.numpy())
    assert got["pos"].dtype == np.float64 and np.array_equal(got["pos"], env._st["pos"])
    assert np.array_equal(got["rot"], env._st["rot"])
    assert got["step_counter"].tolist() == [(1 << 40) + 3] and got["counters"].tolist() == [5, 1, 2, 99]
    budget = 20000  # a row is 4 + 32 + 16 + 8 (its id) bytes: 332 of the 1,000 games fit beside the 40 scalar bytes
    for d in ("s0", "s1"):
        bench.dump_outputs(str(tmp_path / d), env, budget=budget)
    s = {f[:-4]: np.load(tmp_path / "s0" / f) for f in os.listdir(tmp_path / "s0")}
    assert all(np.array_equal(v, np.load(tmp_path / "s1" / f"{k}.npy")) for k, v in s.items())
    g = s["games"].astype(np.int64)
    assert len(g) == 332 and np.all(np.diff(g) > 0) and g[0] >= 0 and g[-1] < n
    assert sum(v.nbytes for v in s.values()) <= budget
    assert np.array_equal(s["pos"], env._st["pos"][g]) and np.array_equal(s["done"], env.bench_done.numpy()[g])
    bench.dump_outputs(str(tmp_path / "r1"), env, rank=1)
    assert sorted(os.listdir(tmp_path / "r1"))[0] == "counters.rank1.npy"


def test_launch_sets_name_the_traced_kernels():
    """the learner roofline names the kernels rocprofv3 reports for each of
    the reference-order tick's launch sets"""
    f = bench._launch_sets("fp32", "param_noise")
    assert f["acting"].startswith("k_act_step32<true>")
    assert "k_grad_slice_bwd<1>" in f["critic_step"] and "k_grad_slice_bwd<2>" in f["actor_step"]
    assert bench._launch_sets("fp32", "action_noise")["acting"].startswith("k_act_step32<false>")
    assert "k_critic_grad<true>" in bench._launch_sets("bf16", "param_noise")["critic_step"]
