"""The fp32 actor's exploration noise, keyed: k_actor_fwd32 / k_actor_fwd16
(csrc/sk_act32.hpp, through ActorKernel32) against oracle/noise_ref.py, the
numpy fp64 restatement of what they draw as a pure function of (seed, call,
global row, unit) -- every row, both outputs, nothing masked out.

Cases (tests/noise_cases.py): a seeded default-init Actor (unsaturated) and one
with biases N(0, 0.1); 67 observation-like rows with entries exactly 0 and 1
(three 32-row / five 16-row tiles, row keys >= 32, a ragged last group), their
first 5 (a ragged second group) and first 1; both tiles (SK_FWD16 = 0 / 1);
noise_sd 0.1 / 0.5 with action_sd 0 / 0.15, and action noise alone; (seed,
counter) = (5, 0) and (0x0123456789ABCDEF, 2^32 - 1), whose first call number
is 2^32, so the high words of seed and call count.  Two consecutive calls per
case match the restatement at call and call + 1; the counter then holds the
last call number, its other words 0.  The 16-row tile is compared with exact
squares in the variance, the 32-row tile with bf16 squares.

Bars: 16 x the restatement's own fp32-against-fp64 error on these inputs
(computed at run time, never from the kernel); the factor allows for the
hardware v_log_f32 / v_sin_f32 / v_cos_f32 and the MFMA's summation order --
supposed, not measured: the hardware transcendentals' accuracy was not
measured separately.  Cap: 1/4 of the deviation a 1 % error in sd makes.

    comparison               floor      bar (16 x)  cap        kernel max
    16-row tile, sd 0.1      1.56e-07   2.50e-06    1.19e-04   9.72e-08
    16-row tile, sd 0.5      1.36e-07   2.18e-06    7.52e-04   1.13e-07
    32-row tile, sd 0.1      2.58e-07   4.13e-06    1.19e-04   1.04e-07
    32-row tile, sd 0.5      3.70e-06   5.91e-05    7.52e-04   1.13e-07
    action normals z         7.28e-07   1.16e-05    5.17e-03   3.68e-07 / 3.30e-07 (32- / 16-row kernel)
    noise-free (3 x floor)   6.83e-08   2.05e-07    4.63e-07   8.46e-08 / 6.88e-08 (32- / 16-row kernel)

(noise-free cap: 0.8 x the least deviation of the split GEMM with one of
x_lo.w_hi, x_hi.w_lo, x_mid.w_mid dropped: 8.67e-07, 5.79e-07, 1.21e-06;
tests/test_noise_ref_cpu.py.)  Run with `-s` for the per-case maxima."""
import copy

import numpy as np
import pytest
import torch

import noise_cases as nc
from oracle import noise_ref as nr
from test_learn32_gpu import _np

pytestmark = pytest.mark.gpu

SEED_IDS = ["seed5_call1", "seed64_call2p32"]


@pytest.fixture(scope="module")
def kit():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from skillshot_learning_amd.actor_kernel import ActorKernel32
    x = torch.from_numpy(nc.inputs().copy()).cuda()
    actors = {net: copy.deepcopy(nc.actor(net)).cuda() for net in nc.NETS}
    return dict(x=x, actors=actors, kernel=ActorKernel32)


@pytest.fixture(params=["0", "1"], ids=["rows32", "rows16"])
def tile(request, monkeypatch):
    """the 32-row tile (bf16 squares in the variance GEMM) and the 16-row
    tile (exact squares)"""
    monkeypatch.setenv("SK_FWD16", request.param)
    return "bf16" if request.param == "0" else "exact"


def _counter_is(k, call):
    torch.cuda.synchronize()
    return int(k._ctr[0]) == call and not k._ctr[1:].any()


@pytest.mark.parametrize("rows", nc.ROW_COUNTS)
@pytest.mark.parametrize("case", [0, 1], ids=SEED_IDS)
@pytest.mark.parametrize("net", nc.NETS)
def test_noisy_forward_matches_keyed_restatement(kit, tile, net, case, rows):
    seed, c0 = nc.SEED_CASES[case]
    bars = nc.bars()
    k = kit["kernel"](kit["actors"][net], seed=seed)
    x = kit["x"][:rows].contiguous()
    missed = []
    for sd in nc.SDS:
        for asd in (0.0, nc.ACTION_SD):
            k._ctr[0] = c0
            worst = 0.0
            for call in nc.calls(c0):
                got = _np(k(x, noise_sd=sd, action_sd=asd))
                want = nc.reference(net, sd, asd, seed, call, tile)[:rows]
                assert got.shape == want.shape
                worst = max(worst, float(np.abs(got - want).max()))
            print(f"{tile} squares, {net}, {rows} rows, seed {seed:#x}, calls {c0 + 1}.., sd {sd}, action_sd {asd}: "
                  f"max |kernel - restatement| {worst:.3g} (bar {bars[tile, sd]:.3g})")
            assert _counter_is(k, c0 + 2)
            if not worst <= bars[tile, sd]:
                missed.append((sd, asd, worst, bars[tile, sd]))
    assert not missed, missed


@pytest.mark.parametrize("rows", nc.ROW_COUNTS)
@pytest.mark.parametrize("case", [0, 1], ids=SEED_IDS)
def test_action_noise_matches_keyed_normals(kit, tile, case, rows):
    """action noise alone: (a1 - clean) / action_sd is the restated z of unit
    385, keyed by the row itself; a launch without noise leaves the counter"""
    seed, c0 = nc.SEED_CASES[case]
    bar = nc.bars()["z"]
    k = kit["kernel"](kit["actors"]["default"], seed=seed)
    x = kit["x"][:rows].contiguous()
    k._ctr[0] = c0
    clean = _np(k(x))
    assert _counter_is(k, c0)
    worst = 0.0
    for call in nc.calls(c0):
        z = (_np(k(x, action_sd=nc.ACTION_SD)) - clean) / nc.ACTION_SD
        worst = max(worst, float(np.abs(z - nr.action_normals(seed, call, np.arange(rows))).max()))
    print(f"{tile} tile, {rows} rows, seed {seed:#x}, calls {c0 + 1}..: max |z - restated z| {worst:.3g} (bar {bar:.3g})")
    assert _counter_is(k, c0 + 2)
    assert worst <= bar, (worst, bar)


@pytest.mark.parametrize("rows", nc.ROW_COUNTS)
@pytest.mark.parametrize("net", nc.NETS)
def test_noise_free_forward_sees_a_dropped_piece_product(kit, tile, net, rows):
    """the noise-free forward on the same unsaturated nets against
    keras_ref.actor_forward, at a bar (3 x the restatement's fp32 error) below
    0.8 x what the loss of any one class of the split GEMM's piece products
    costs (tests/test_noise_ref_cpu.py)"""
    bar = nc.bars()["clean"]
    k = kit["kernel"](kit["actors"][net], seed=1)
    got = _np(k(kit["x"][:rows].contiguous()))
    err = float(np.abs(got - nc.clean_reference(net)[:rows]).max())
    print(f"{tile} tile, {net}, {rows} rows: max |kernel - fp64| {err:.3g} (bar {bar:.3g})")
    assert err <= bar, (err, bar)
