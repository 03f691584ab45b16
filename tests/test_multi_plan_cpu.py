"""Which multi-tick kernel a launch runs (plan_multi, csrc/sk_multi_plan.hpp):
the decision alone, through skdiag_multi_plan, no device.  Every path of the
multi-tick step is exact, so a slipped threshold or a wrong fallback under
stream capture would pass every GPU test and only slow the benchmark; here
each decision is pinned.

tests/golden/multi_plan.npz holds the decisions of the launch code that
plan_multi replaced (commit `parent` in the file), recorded from that code
with its HIP calls replaced by the inputs pack_allowed and planes_fit32.  Its
rows are the product of
  n        every threshold and its neighbours, and the 48 n / 16 n 32-bit bounds
  n_ticks  1, 2, 20, 99, 100, 400
  full     step-only / the full contract
  flags    restart_fits, pack_allowed, planes_fit32, steady_ok: all set, one
           cleared at a time, all cleared
  knobs    the defaults; every SK_MULTI_* knob alone through -1, 0, 1, 2, 3, 4,
           7, 64, 128, 256, 512; split x pack, block x prefetch, pack x fast
stored field-major: plan[field, n, n_ticks, full, flags, knobs].
"""
import ctypes
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multi_plan.npz")

# skdiag_multi_plan's field order (sk_engine.hip)
IN_FIELDS = ["n", "n_ticks", "full", "restart_fits", "pack_allowed", "planes_fit32", "steady_ok",
             "policy", "split", "early", "block", "stagger", "prefetch", "pack", "fast"]
OUT_FIELDS = ["split", "pol", "blk", "obs", "pf", "pack", "fast", "stagger", "early", "steady32", "grid",
              "block_threads"]
DEFAULTS = dict(full=0, restart_fits=1, pack_allowed=1, planes_fit32=1, steady_ok=1,
                policy=1, split=-1, early=-1, block=-1, stagger=0, prefetch=-1, pack=-1, fast=-1)


@pytest.fixture(scope="module")
def plan_rows():
    import skillshot_learning_amd as m
    f = m.load_library().skdiag_multi_plan
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    f.restype = ctypes.c_int

    def rows(inputs):
        inputs = np.ascontiguousarray(inputs, dtype=np.int64)
        out = np.full((inputs.shape[0], len(OUT_FIELDS)), -99, dtype=np.int32)
        for i in range(inputs.shape[0]):
            assert f(inputs[i].ctypes.data, out[i].ctypes.data) == 0
        return out
    return rows


@pytest.fixture(scope="module")
def plan(plan_rows):
    def one(n, n_ticks, **kw):
        assert set(kw) <= set(DEFAULTS)
        v = dict(DEFAULTS, n=n, n_ticks=n_ticks, **kw)
        return dict(zip(OUT_FIELDS, plan_rows([[v[k] for k in IN_FIELDS]])[0].tolist()))
    return one


def test_every_row_of_the_recorded_table(plan_rows):
    z = np.load(GOLDEN)
    assert z["in_fields"].tolist() == IN_FIELDS and z["out_fields"].tolist() == OUT_FIELDS
    assert len(str(z["parent"])) == 40
    axes = [z["n"], z["n_ticks"], z["full"], z["flags"], z["knobs"]]
    assert z["n"].tolist() == [1, 8192, 8193, 32768, 32769, 40959, 40960, 65535, 65536, 65537, 98304, 98305, 131072,
                               89478485, 89478486, 134217727]
    assert z["n_ticks"].tolist() == [1, 2, 20, 99, 100, 400] and z["full"].tolist() == [0, 1]
    want = z["plan"]
    assert want.shape == (len(OUT_FIELDS),) + tuple(len(a) for a in axes)
    idx = np.indices(want.shape[1:]).reshape(5, -1)
    inputs = np.concatenate([axes[0][idx[0], None], axes[1][idx[1], None], axes[2][idx[2], None],
                             axes[3][idx[3]], axes[4][idx[4]]], axis=1)
    assert inputs.shape == (want[0].size, len(IN_FIELDS))
    got = plan_rows(inputs)
    for j, name in enumerate(OUT_FIELDS):
        bad = np.flatnonzero(got[:, j] != want[j].reshape(-1))
        assert bad.size == 0, (name, dict(zip(IN_FIELDS, inputs[bad[0]].tolist())), int(got[bad[0], j]),
                               int(want[j].reshape(-1)[bad[0]]))


def test_the_defaults_the_readme_names(plan):
    # step-only, the benchmark's 65,536 games x 400 ticks: the packed split kernel on the fp32-trig tick
    p = plan(65536, 400)
    assert p == dict(split=1, pol=1, blk=64, obs=0, pf=0, pack=1, fast=1, stagger=0, early=0, steady32=1,
                     grid=2048, block_threads=64)
    # ... at 20 ticks per launch on the fp64 carry
    assert plan(65536, 20) == dict(p, fast=0)
    assert plan(98304, 400) == dict(p, grid=3072)
    # 32,768 games: split, the 88-B form, the prefetch wave 2 ticks ahead
    assert plan(32768, 400) == dict(split=1, pol=1, blk=64, obs=0, pf=2, pack=0, fast=0, stagger=0, early=0,
                                    steady32=1, grid=1024, block_threads=128)
    assert plan(8192, 400) == dict(split=1, pol=1, blk=64, obs=0, pf=0, pack=0, fast=0, stagger=0, early=0,
                                   steady32=1, grid=256, block_threads=64)
    # 131,072 games: one lane per game, packed, four waves per workgroup, the early restart draw
    assert plan(131072, 400) == dict(split=0, pol=1, blk=256, obs=0, pf=0, pack=1, fast=0, stagger=0, early=1,
                                     steady32=1, grid=512, block_threads=256)
    # the full contract: always split; 512-lane workgroups with the prefetch wave 4 ticks ahead from 65,536 games
    assert plan(65536, 400, full=1) == dict(split=1, pol=1, blk=512, obs=1, pf=4, pack=0, fast=0, stagger=0, early=0,
                                            steady32=1, grid=256, block_threads=576)
    assert plan(32768, 400, full=1) == dict(split=1, pol=1, blk=64, obs=1, pf=0, pack=0, fast=0, stagger=0, early=0,
                                            steady32=1, grid=1024, block_threads=64)
    # a capturing stream and no pack buffer: one lane per game on the 88-B form
    assert plan(65536, 400, pack_allowed=0) == dict(split=0, pol=1, blk=256, obs=0, pf=0, pack=0, fast=0, stagger=0,
                                                    early=1, steady32=1, grid=256, block_threads=256)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 65])
def test_the_gpu_tests_forcing_reaches_the_packed_split_kernel(plan, n):
    """tests/multi_split_cases.py's _env at the sizes of tests/test_multi_split_*_gpu.py: exactly
    k_step_split_multi<p, b, false, 0, true, f> with the steady loop allowed."""
    for p in (0, 1):
        for b in (64, 512):
            for f in (0, 1):
                assert plan(n, 12, split=1, pack=1, fast=f, policy=p, block=b) == dict(
                    split=1, pol=p, blk=b, obs=0, pf=0, pack=1, fast=f, stagger=0, early=0, steady32=1,
                    grid=(2 * n + b - 1) // b, block_threads=b)


def test_odd_knob_values_fall_as_they_always_did(plan):
    assert plan(65536, 400, block=128) == plan(65536, 400)
    assert plan(131072, 400, block=128) == dict(plan(131072, 400), blk=64, grid=2048, block_threads=64)
    assert plan(32768, 400, prefetch=3)["pf"] == 4 and plan(32768, 400, prefetch=7)["pf"] == 4
    assert plan(65536, 400, split=0, pack=0, block=64, prefetch=3) == dict(
        split=0, pol=1, blk=64, obs=0, pf=4, pack=0, fast=0, stagger=0, early=1, steady32=1, grid=1024,
        block_threads=128)
    assert plan(65536, 400, policy=2)["pol"] == 0 and plan(65536, 400, planes_fit32=0)["pol"] == 0


def test_bad_arguments_are_refused(plan_rows):
    import skillshot_learning_amd as m
    f = m.load_library().skdiag_multi_plan
    out = (ctypes.c_int32 * 12)()
    row = (ctypes.c_int64 * 15)(0, 1, 0, 1, 1, 1, 1, 1, -1, -1, -1, 0, -1, -1, -1)
    assert f(row, out) != 0
    assert f(None, out) != 0
