"""oracle/noise_ref.py, the keyed restatement of the fp32 actor's exploration
noise, pinned on the CPU: its Philox against rng.philox4x32_10 and the
Random123 known answers, its noisy forward against explicit weight noise
(SkillshotLearner.py:245-281), and the floors, mutant deviations and bars that
tests/test_actor_noise_keyed_gpu.py compares the kernels with (computed from
the restatement alone, tests/noise_cases.py; printed with `pytest -s`).

Each fault a keyed generator can have without moving its marginal statistics
is restated here as a mutant of the reference's normals (`_xi`): every one has
to miss the reference by at least 4 x the bar the kernel is held to."""
import math

import numpy as np
import pytest
import torch

import noise_cases as nc
from oracle import keras_ref as kr
from oracle import noise_ref as nr
from skillshot_learning_amd import rng

U32 = 0xFFFFFFFF
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def _round(c, k):
    """one Philox4x32 round on Python ints"""
    p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
    return [(p1 >> 32) ^ c[1] ^ k[0], p1 & U32, (p0 >> 32) ^ c[3] ^ k[1], p0 & U32]


def _rounds(c, k, n):
    c, k = list(c), list(k)
    for _ in range(n):
        c = _round(c, k)
        k = [(k[0] + 0x9E3779B9) & U32, (k[1] + 0xBB67AE85) & U32]
    return c


def test_philox_rounds():
    """10 rounds: the known answers of tests/test_oracle_golden.py and
    rng.philox4x32_10 on arrays.  The round count is a loop bound, so no
    vectors are invented for 7 rounds: they are the same round function,
    written out here on Python ints, applied seven times."""
    for ctr, key, want in KAT:
        assert tuple(int(x) for x in nr.philox4x32(*ctr, *key, rounds=10)) == want
        assert _rounds(ctr, key, 10) == list(want)
        assert [int(x) for x in nr.philox4x32(*ctr, *key, rounds=7)] == _rounds(ctr, key, 7)
    r = np.random.RandomState(0)
    c = r.randint(0, 2 ** 32, size=(4, 257), dtype=np.uint64)
    k0, k1 = 0x89ABCDEF, 0x01234567
    want = rng.philox4x32_10(*[torch.from_numpy(x.astype(np.int64)) for x in c], k0, k1)
    got = nr.philox4x32(*c, k0, k1)
    for g, w in zip(got, want):
        assert np.array_equal(g.astype(np.int64), w.numpy())
    got7 = nr.philox4x32(*c, k0, k1, rounds=7)
    for j in (0, 100, 256):
        assert [int(x[j]) for x in got7] == _rounds([int(x[j]) for x in c], (k0, k1), 7)
    # the keying: counter (row_key, unit, call lo, call hi), key (seed lo, seed hi)
    seed, call = 0x0123456789ABCDEF, (7 << 32) | 9
    w = nr.draw_words(seed, call, np.array([40]), 300, 7)[0]
    assert [int(x) for x in w] == _rounds([40, 300, 9, 7], [0x89ABCDEF, 0x01234567], 7)


def test_normals4_definition():
    """u1 = ((w >> 8) + 0.5) 2^-24 in fp32: exact up to 2^23, rounded to even
    above it, the top bucket exactly 1.0 (z = 0); u2 in revolutions; the pair
    order [r cos, r sin]"""
    w = np.array([[0, 0, (2 ** 24 - 1) << 8, 1 << 30], [(2 ** 23 + 1) << 8, 1 << 31, (2 ** 23 + 2) << 8 | 0xFF, 3 << 30]],
                 dtype=np.uint64)
    u1, u2 = nr.uniforms(w)
    assert u1.dtype == np.float32 and u2.dtype == np.float32
    assert u1[0, 0] == np.float32(2.0 ** -25) and u1[0, 1] == np.float32(1.0)
    assert u1[1, 0] == np.float32((2 ** 23 + 2) * 2.0 ** -24)  # 2^23 + 1.5 -> even
    assert u1[1, 1] == np.float32((2 ** 23 + 2) * 2.0 ** -24)  # 2^23 + 2.5 -> even
    assert list(u2.ravel()) == [0.0, 0.25, 0.5, 0.75]
    z = nr.normals4(w)
    r0 = math.sqrt(-2.0 * math.log(2.0 ** -25))
    assert abs(z[0, 0] - r0) < 1e-12 and abs(z[0, 1]) < 1e-12  # angle 0: (r, 0)
    assert z[0, 2] == 0.0 and z[0, 3] == 0.0  # u1 = 1: radius 0
    r1 = math.sqrt(-2.0 * math.log(float(u1[1, 0])))
    assert abs(z[1, 0] + r1) < 1e-12 and abs(z[1, 1]) < 1e-12  # half a revolution: (-r, 0)
    assert abs(z[1, 2]) < 1e-12 and abs(z[1, 3] + r1) < 1e-12  # three quarters: (0, -r)


def test_bf16_round_and_split():
    r = np.random.RandomState(1)
    v = (r.randn(4096) * np.exp(r.randn(4096) * 3)).astype(np.float32)
    v[:4] = [0.0, 1.0, 1.00390625, 1.01171875]  # ties: 1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6
    want = torch.from_numpy(v).to(torch.bfloat16).float().numpy()
    assert np.array_equal(nr.bf16_round(v), want)
    hi, mid, lo = nr.split3(v)
    assert np.abs(v.astype(np.float64) - (hi + mid + lo)).max() <= 2.0 ** -24 * np.abs(v).max()
    assert (np.abs(v.astype(np.float64) - (hi + mid + lo)) <= 2.0 ** -25 * np.abs(v) + 1e-300).all()


def test_zero_noise_reduces_to_keras():
    for net in nc.NETS:
        want, _ = kr.actor_forward(nc.params(net), nc.inputs().astype(np.float64))
        got = nr.actor_forward_noisy(nc.params(net), nc.inputs(), 0.0, 0.0, seed=9, call=3)
        assert np.array_equal(got, want)
        assert np.array_equal(nc.reference(net, 0.0, 0.0, 0, 0, "exact"), want)


def _ks2(a, b):
    """two-sample Kolmogorov-Smirnov distance"""
    a, b = np.sort(a), np.sort(b)
    grid = np.concatenate([a, b])
    return float(np.abs(np.searchsorted(a, grid, side="right") / a.size
                        - np.searchsorted(b, grid, side="right") / b.size).max())


@pytest.mark.parametrize("state", [0, 1])
def test_restated_noise_has_reference_distribution(state):
    """model_act_param_noise (SkillshotLearner.py:245-281) per sample: 4,096
    restated rows of one state (distinct row keys) against explicit weight
    noise w (1 + 0.5 N(0,1)) drawn per sample in fp64; two-sample KS per
    output at the level of test_actor_forward_f32_param_noise_distribution"""
    n, sd = 4096, 0.5
    P = nc.params("biased")
    x = nc.inputs()[[11, 40][state]].astype(np.float64)
    got = nr.actor_forward_noisy(P, np.broadcast_to(x, (n, 12)), sd, 0.0, seed=77 + state, call=1 + state,
                                 row0=64 * state)
    r = np.random.RandomState(5 + state)
    outs = []
    for _ in range(n // 256):
        h = np.broadcast_to(x, (256, 12))
        for j, l in enumerate(("l1", "l2", "l3")):
            W, b = P[l + ".weight"], P[l + ".bias"]
            Wn = W[None] * (1 + sd * r.standard_normal((256,) + W.shape))
            bn = b[None] * (1 + sd * r.standard_normal((256,) + b.shape))
            h = np.einsum("boi,bi->bo", Wn, h) + bn
            h = np.tanh(h) if j == 2 else np.maximum(h, 0)
        outs.append(h)
    ex = np.concatenate(outs)
    for j in range(2):
        d = _ks2(got[:, j], ex[:, j])
        print(f"state {state} output {j}: KS {d:.4f} (bar {1.95 * math.sqrt(2 / n) * 1.3:.4f}), "
              f"std {got[:, j].std():.4f} / {ex[:, j].std():.4f}")
        assert got[:, j].std() > 1e-3  # the noise moves the output: the comparison is not vacuous
        assert d < 1.95 * math.sqrt(2 / n) * 1.3


# ---------------------------------------------------------------- mutants
# fault -> the rows it leaves keyed as before (None: it rekeys every row)
KEY_FAULTS = {
    "same_pair": lambda r: r % 4 < 2,     # rows 2, 3 of a group read rows 0, 1's Box-Muller pair
    "row_key": lambda r: r % 4 == 0,      # the group's draw keyed by the row, not by 4 (row // 4)
    "layer2_unit": None,                  # layer 2 keyed like layer 1 (u, not 256 + u)
    "cos_sin": None,                      # the pair's order swapped
    "call_hi": None,                      # the call number's high word ignored
    "seed_hi": None,                      # the seed's high word ignored
    "tile_local": lambda r: r < 16,       # rows keyed within their 16-row tile: the two tiles' streams differ
    "rounds_hidden": None,                # layers 1 / 2 with 10 rounds
    "rounds_l3": None,                    # layer 3 with 7 rounds
}


def _xi(seed, call, rows, fault=None):
    """the reference's parameter normals, restated with one fault"""
    s = seed & U32 if fault == "seed_hi" else seed
    c = call & U32 if fault == "call_hi" else call
    rows = np.asarray(rows, dtype=np.uint64)
    key = rows % np.uint64(16) if fault == "tile_local" else rows

    def z_of(k, unit, rounds):
        z = nr.normals4(nr.draw_words(s, c, k, unit, rounds))
        return z[..., [1, 0, 3, 2]] if fault == "cos_sin" else z

    def hidden(unit0, units):
        u = np.arange(units, dtype=np.uint64)[None, :] + np.uint64(unit0)
        k = key[:, None] if fault == "row_key" else key[:, None] & ~np.uint64(3)
        z = z_of(k, u, 10 if fault == "rounds_hidden" else 7)
        pick = (key % np.uint64(4)).astype(np.int64)
        if fault == "same_pair":
            pick = pick & 1
        return np.take_along_axis(z, np.broadcast_to(pick[:, None, None], z.shape[:-1] + (1,)), -1)[..., 0]

    return (hidden(0, 256), hidden(0 if fault == "layer2_unit" else 256, 128),
            z_of(key, nr.UNIT_L3, 7 if fault == "rounds_l3" else 10)[..., :2])


def _row_dev(got, want):
    return np.abs(got - want).max(axis=1)


def test_mutant_builder_restates_the_reference():
    rows = np.arange(nc.ROWS)
    for seed, c0 in nc.SEED_CASES:
        for a, b in zip(_xi(seed, c0 + 1, rows), nr.param_normals(seed, c0 + 1, rows)):
            assert np.array_equal(a, b)


def test_floors_mutants_and_bars():
    """The floors (fp32 run of the restatement against its fp64 run), the
    bars (16 x floor) and caps (1/4 of the 1 %-sd mutant), and every fault's
    deviation from the reference on the GPU test's inputs: a keying fault
    moves at least 90 % of the rows it rekeys by 4 x the bar or more (the rows
    it leaves keyed as before -- the first row of a group under the row-key
    fault, the first tile under the tile-local one -- are exactly unchanged,
    so the 90 % is of the rekeyed rows); a 1 % error in sd, a variance 3 % off
    and every keying fault miss the comparison by at least 4 x its bar."""
    f, caps, bars = nc.floors(), nc.caps(), nc.bars()
    print("floors (max |fp32 - fp64|):", {str(k): f"{v:.3g}" for k, v in f.items()})
    print("bars:", {str(k): f"{v:.3g}" for k, v in bars.items()})
    print("caps:", {str(k): f"{v:.3g}" for k, v in caps.items()})
    for sd in nc.SDS:
        for sq in ("exact", "bf16"):
            assert 0 < bars[sq, sd] <= caps[sd], (sq, sd, bars[sq, sd], caps[sd])
    assert 0 < bars["z"] <= caps["z"]
    rows = np.arange(nc.ROWS)
    X = nc.inputs()
    seed, c0 = nc.SEED_CASES[1]  # call = 2^32 and a seed above 2^32: both high words count
    call = c0 + 1
    assert call == 2 ** 32 and seed >> 32
    for net in nc.NETS:
        P = nc.params(net)
        for sd in nc.SDS:
            for sq in ("exact", "bf16"):
                want, bar = nc.reference(net, sd, 0.0, seed, call, sq), bars[sq, sd]
                for fault, same in KEY_FAULTS.items():
                    got = nr.forward_with_normals(P, X, sd, _xi(seed, call, rows, fault), squares=sq)
                    dev = _row_dev(got, want)
                    keep = same(rows) if same else np.zeros(nc.ROWS, dtype=bool)
                    frac = float((dev[~keep] >= 4 * bar).mean())
                    print(f"{net} sd {sd} {sq:5s} {fault:13s}: max {dev.max():.3g}, least rekeyed row "
                          f"{dev[~keep].min():.3g}, {100 * frac:.0f} % of {int((~keep).sum())} rekeyed rows "
                          f">= 4 x bar {bar:.3g}")
                    assert not dev[keep].any(), (net, sd, sq, fault)
                    assert frac >= 0.9, (net, sd, sq, fault, frac)
                    assert dev.max() >= 4 * bar
                xi = nr.param_normals(seed, call, rows)
                for name, got in (("sd x 1.01", nr.forward_with_normals(P, X, sd * 1.01, xi, squares=sq)),
                                  ("variance x 1.03", nr.forward_with_normals(P, X, sd, xi, squares=sq,
                                                                              var_scale=1.03))):
                    dev = _row_dev(got, want)
                    print(f"{net} sd {sd} {sq:5s} {name:15s}: max {dev.max():.3g} (4 x bar {4 * bar:.3g})")
                    assert dev.max() >= 4 * bar, (net, sd, sq, name)
                # the other tile's squares are not this tile's reference
                other = nc.reference(net, sd, 0.0, seed, call, "bf16" if sq == "exact" else "exact")
                print(f"{net} sd {sd} {sq:5s} other squares  : max {_row_dev(other, want).max():.3g}")
                assert _row_dev(other, want).max() > bar, (net, sd, sq)
    # action noise: the normals are what the action-only comparison sees
    za = nr.action_normals(seed, call, rows)
    for name, got in (("cos_sin", za[:, ::-1]), ("call_hi", nr.action_normals(seed, call & U32, rows)),
                      ("seed_hi", nr.action_normals(seed & U32, call, rows)),
                      ("unit", nr.row_normals(seed, call, rows, nr.UNIT_L3)),
                      ("action_sd x 1.01", 1.01 * za)):
        dev = _row_dev(got, za)
        print(f"action normals {name:16s}: max {dev.max():.3g} (4 x bar {4 * bars['z']:.3g})")
        assert dev.max() >= 4 * bars["z"], name


def test_noise_free_bar_sees_a_dropped_piece_product():
    """the noise-free bar (CLEAN_FACTOR x E_clean) lies below 0.8 x the
    deviation of the split GEMM (three bf16 pieces per operand, sk_split.hpp's
    six products, fp64 sums) with any one of x_lo.w_hi, x_hi.w_lo, x_mid.w_mid
    dropped, and above the six-product model's own error"""
    f, bars, d = nc.floors(), nc.bars(), nc.dropped_deviations()
    print(f"E_clean {f['clean']:.3g}, bar {bars['clean']:.3g}; six products {d['full']:.3g}; dropped:",
          {k: f"{v:.3g}" for k, v in d.items() if k != "full"})
    for net in nc.NETS:
        a = np.abs(nc.clean_reference(net))
        print(f"{net}: |a| max {a.max():.3g}, median {np.median(a):.3g}")
        assert a.max() < 0.7  # unsaturated: tanh does not hide the pre-activation's error
    assert d["full"] <= bars["clean"]
    for name in nc.DROPPED:
        assert d[name] > bars["clean"], name
        assert bars["clean"] < 0.8 * d[name], name
