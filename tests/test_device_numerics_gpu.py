"""The step engine's numeric primitives as the device compiles them, element by
element through the probe kernels (oracle/sk_probe.hip: the product headers
built with the product's flag list), on the inputs of tests/numerics_cases.py.

1. Device == host twin, bit for bit, values and flags, for every
   host-compilable group (sk_trig.hpp, sk_tan_cr.hpp, sk_range.hpp) over the
   full input sets and 2^20 random inputs each: every bound the CPU checks
   establish (tests/trig_check.cpp, tan_cr_check.cpp, fast_step_check.cpp,
   pair_collision_check.cpp, steady_admit_check.cpp) then holds on the device.
2. Device against references that do not pass through the twin: the 70-digit
   Decimal sin / cos / tan of tests/cr_tan.py, glibc's sin / cos (the
   reference's), Python's %, integer restatements.  Bars:
     tan_cr, grad_cr      == cr_tan bit for bit
     sincos_bf            <= 1 ulp from math.sin / math.cos, exact at +-0
     sincos_fast          <= SKT_FAST_ERR / 2;  sincos_add <= SKT_ADD_ERR / 2
     ok                   false exactly outside the range and for non-finite input
     sincos_lib           <= 1 ulp from math.sin / math.cos on 1.6e6 .. 1e15
     grad_fast, tan_lib   relative error against cr_tan <= 2^-42, a quarter of
                          future_collision_s' kFutureMargin = 2^-40 (the rest
                          is for the roundings of yi, v0 and v1)
     dist_point_point     == the correctly rounded sqrt of the exact integer sum
     dist_line_point      == the expression in numpy fp64, the reference's order
     py_mod2*             == Python's r % 2 for every finite r, NaN otherwise
     philox4x32_10, u32_to_action, u32_to_pos, the range predicates: exact
3. One state through the engine: rotations of -5e-324, -1e-323, -0.0 and -1e-20
   observed on the GPU and on the CPU backend.

No launch has more than 2^20 elements.
"""
import math

import numpy as np
import pytest
import torch

import numerics_cases as nc
from oracle import noise_ref, probe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")

    def run(group, **inputs):
        return nc.in_chunks(probe.run_device, group, probe.MAX_ELEMENTS, **inputs)
    return run


def _host(group, **inputs):
    return nc.in_chunks(probe.run_host, group, probe.MAX_ELEMENTS, **inputs)


def _assert_twin(group, inputs, got):
    want = _host(group, **inputs)
    bad = nc.twin_differences(group, inputs, got, want)
    n = next(iter(inputs.values())).shape[-1]  # (an index into a [planes, n] output is flat)
    assert not bad, (len(bad), [(name, i, {k: repr(v[..., i % n]) for k, v in inputs.items()},
                                 repr(got[name].ravel()[i]), repr(want[name].ravel()[i])) for name, i in bad[:4]])


# ---------------------------------------------------------------- 1. the twin
@pytest.mark.parametrize("which", ["sets", "random"])
def test_trig_equals_host_twin(dev, which):
    inputs = nc.trig_inputs(1 << 18) if which == "sets" else nc.random_trig_inputs()
    got = dev("trig", **inputs)
    ok = got["fast_ok"] != 0
    assert ok.sum() > 0.7 * ok.size and (~ok).sum() > 10  # values are compared where ok, flags everywhere
    _assert_twin("trig", inputs, got)


@pytest.mark.parametrize("which", ["sets", "random"])
def test_tan_cr_equals_host_twin(dev, which):
    if which == "sets":  # the angles as arguments and as rotations (the game's argument is -rot + pi/2)
        a = nc.angles(1 << 16)
        x = np.concatenate([a, -a + math.pi / 2])
    else:
        x = np.random.default_rng(14).uniform(-nc.TAN_CR_MAX, nc.TAN_CR_MAX, 1 << 20)
    _assert_twin("tan", dict(x=x), dev("tan", x=x))


def test_range_predicates_equal_host_twin_and_their_definitions(dev):
    t = nc.range_tuples()
    got = dev("range", v=t)
    _assert_twin("range", dict(v=t), got)
    want, defined = nc.range_definitions(t)
    bad = np.argwhere((got["out"] != want) & defined)
    assert bad.size == 0, [(probe.RANGE_PREDICATES[k], t[:, i].tolist()) for k, i in bad[:5]]


# ---------------------------------------------------------------- 2. independent references
def test_sincos_against_decimal_and_glibc(dev):
    inp = {k: v[:nc.crafted_angles().size] for k, v in nc.trig_inputs(1 << 12).items()}
    x = inp["x"] = nc.crafted_angles()
    d = inp["d"].astype(np.float64)
    out = dev("trig", **inp)
    ref = nc.crafted_reference()
    ok = np.abs(x) < nc.FAST_MAX  # false for NaN
    assert np.array_equal(out["bf_ok"] != 0, ok) and np.array_equal(out["fast_ok"] != 0, ok)
    assert (~ok).sum() >= 15 and ok.sum() >= 1800
    us = nc.ulps(out["bf_s"][ok], np.array([math.sin(v) for v in x[ok]]))
    uc = nc.ulps(out["bf_c"][ok], np.array([math.cos(v) for v in x[ok]]))
    ef = max(np.abs(out["fast_s"][ok].astype(np.float64) - ref["sin"][ok]).max(),
             np.abs(out["fast_c"][ok].astype(np.float64) - ref["cos"][ok]).max())
    from cr_tan import cr_sincos
    sd = np.array([cr_sincos(v) for v in (x[ok] + d[ok]).tolist()])  # the fp64 rotation after the look
    ea = max(np.abs(out["add_s"][ok].astype(np.float64) - sd[:, 0]).max(),
             np.abs(out["add_c"][ok].astype(np.float64) - sd[:, 1]).max())
    print(f"device: sincos_bf max {max(us.max(), uc.max()):.0f} ulp from glibc, sincos_fast max error {ef:.3e}, "
          f"sincos_add {ea:.3e} over {ok.sum()} angles")
    assert us.max() <= 1 and uc.max() <= 1
    zero = np.flatnonzero(x == 0)
    assert zero.size >= 2 and np.signbit(x[zero]).any() and not np.signbit(x[zero]).all()
    assert not nc.bit_differences(out["bf_s"][zero], x[zero]).size  # sin(+-0) = +-0, cos = 1
    assert not nc.bit_differences(out["bf_c"][zero], np.ones(zero.size)).size
    assert ef <= nc.SKT_FAST_ERR / 2
    assert ea <= nc.SKT_ADD_ERR / 2


def test_tan_cr_and_grad_cr_equal_the_decimal_tan(dev):
    x = nc.crafted_angles()
    out = dev("tan", x=x)
    ref = nc.crafted_reference()
    inside = np.abs(x) < nc.TAN_CR_MAX
    assert inside.sum() >= 1600  # (a third of the whole-range sweep lies past 2^20)
    bad = nc.bit_differences(out["tan_cr"], ref["tan"], inside)
    assert bad.size == 0, [(repr(x[i]), repr(out["tan_cr"][i]), repr(ref["tan"][i])) for i in bad[:5]]
    inside = np.abs(-x + math.pi / 2) < nc.TAN_CR_MAX
    bad = nc.bit_differences(out["grad_cr"], ref["grad"], inside)
    assert bad.size == 0, [(repr(x[i]), repr(out["grad_cr"][i]), repr(ref["grad"][i])) for i in bad[:5]]
    g = out["grad_cr"]  # the gradients of the multiples of pi/4: 0, +-1 up to pi's rounding, tan(fl(pi/2))
    assert (g == 0.0).any() and (g == 1.633123935319537e16).any()
    assert (np.abs(g - 1.0) < 1e-15).any() and (np.abs(g + 1.0) < 1e-15).any()


def test_grad_fast_and_tan_lib_stay_inside_the_future_margin(dev):
    """Measured on an MI355X over the crafted angles (finite ones, up to 1e15): grad_fast 2.35e-16 = 2^-51.9,
    tan_lib 2.22e-16 = 2^-52.0; the bar is the code's own constant, not these."""
    x = nc.crafted_angles()
    out = dev("tan", x=x)
    ref = nc.crafted_reference()
    fin = np.isfinite(x)
    rg = nc.relative_error(out["grad_fast"][fin], ref["grad"][fin])
    rt = nc.relative_error(out["tan_lib"][fin], ref["tan"][fin])
    far = np.abs(-x[fin] + math.pi / 2) >= nc.FAST_MAX
    assert far.sum() >= 8 and (~far).sum() >= 1800  # grad_fast's both branches
    print(f"device: grad_fast max relative error {rg.max():.3e} = 2^{math.log2(max(rg.max(), 1e-300)):.1f} "
          f"(past the fast range {rg[far].max():.3e}), tan_lib {rt.max():.3e} = "
          f"2^{math.log2(max(rt.max(), 1e-300)):.1f} over {fin.sum()} angles")
    assert nc.GRAD_BAR == nc.K_FUTURE_MARGIN / 4
    assert rg.max() <= nc.GRAD_BAR
    assert rt.max() <= nc.GRAD_BAR
    assert np.isnan(out["grad_fast"][~fin]).all() and np.isnan(out["tan_lib"][~fin]).all()


def test_sincos_lib_within_one_ulp_of_glibc_past_the_fast_range(dev):
    """The routine the exact ticks call from 1.6e6 rad feeds the same roundings as sincos_bf, so the same bar.
    Measured on an MI355X: 1 ulp at most, 9,125 of 360,472 values off by it."""
    x = nc.lib_angles(1 << 17)
    out = dev("lib", x=x)
    us = nc.ulps(out["s"], np.sin(x))  # numpy's fp64 sin / cos are the C library's, as math.sin / math.cos
    uc = nc.ulps(out["c"], np.cos(x))
    sample = np.random.default_rng(15).choice(x.size, 4096, replace=False)
    assert np.array_equal(np.sin(x[sample]), [math.sin(v) for v in x[sample]])
    assert np.array_equal(np.cos(x[sample]), [math.cos(v) for v in x[sample]])
    print(f"device: sincos_lib max {max(us.max(), uc.max()):.0f} ulp from glibc over {x.size} arguments "
          f"({(us > 0).sum() + (uc > 0).sum()} values differ)")
    assert us.max() <= 1 and uc.max() <= 1
    bad = dev("lib", x=np.array([math.nan, math.inf, -math.inf]))
    assert np.isnan(bad["s"]).all() and np.isnan(bad["c"]).all()


def test_py_mod2_equals_pythons(dev):
    r = nc.mod2_values()
    out = dev("feat", r=r)
    want = nc.py_mod2(r)
    fin = np.isfinite(r)
    for name in ("mod2", "mod2_fast"):
        bad = nc.bit_differences(out[name], want, fin)
        assert bad.size == 0, (name, [(repr(r[i]), repr(out[name][i]), repr(want[i])) for i in bad[:5]])
        assert np.isnan(out[name][~fin]).all() and (~fin).sum() == 3, name


def test_dist_point_point_is_the_correctly_rounded_root(dev):
    p = nc.dist_points()
    got = dev("feat", p=p)["dpp"]
    want = nc.cr_dist_point_point(p)
    q = p.astype(np.int64)
    exact = (q[0] - q[2]) ** 2 + (q[1] - q[3]) ** 2  # < 2^42: exact in fp64 too
    assert np.array_equal(want, [math.sqrt(v) for v in exact.tolist()])
    bad = nc.bit_differences(got, want)
    assert bad.size == 0, [(p[:, i].tolist(), repr(got[i]), repr(want[i])) for i in bad[:5]]


def test_dist_line_point_equals_numpy_in_the_references_order(dev):
    g, p = nc.line_points()
    got = dev("feat", g=g, p=p)["dlp"]
    want = nc.np_dist_line_point(g, p)
    fin = np.isfinite(g)
    assert np.isfinite(want[fin]).all() and fin.sum() > 14000
    bad = nc.bit_differences(got, want, fin)
    assert bad.size == 0, [(repr(g[i]), p[:, i].tolist(), repr(got[i]), repr(want[i])) for i in bad[:5]]
    assert np.isnan(got[~fin]).all()


def test_clamp_action(dev):
    a, af = nc.clamp_values()
    out = dev("feat", a=a, af=af)
    assert not nc.bit_differences(out["clamp"], nc.clamp(a)).size  # a NaN and a -0.0 pass through unchanged
    assert not nc.bit_differences(out["clamp_f"], nc.clamp(af)).size
    assert np.isnan(out["clamp"]).sum() == 1 and np.isnan(out["clamp_f"]).sum() == 1


def test_philox_and_its_conversions_equal_the_integer_restatement(dev):
    ctr, key = nc.rng_words()
    n = ctr.shape[1]
    u, lo, hi = nc.pos_draws()
    out = dev("rng", ctr=ctr, key=key)
    for k0, k1 in {(int(a), int(b)) for a, b in key.T[:64].tolist()} | {(int(key[0, -1]), int(key[1, -1]))}:
        sel = (key[0] == k0) & (key[1] == k1)  # noise_ref's restatement takes one key per call
        want = np.stack(noise_ref.philox4x32(*ctr[:, sel].astype(np.uint64), k0, k1, rounds=10)).astype(np.uint32)
        assert np.array_equal(out["out"][:, sel], want), (k0, k1)
    # every random key: the restatement with per-element keys (the same rounds, keys as arrays)
    want = _philox_per_element(ctr, key)
    assert np.array_equal(out["out"], want)
    assert n > 1 << 16
    out = dev("rng", u=u, lo=lo, hi=hi)
    assert np.array_equal(out["pos"], nc.np_u32_to_pos(u, lo, hi))
    assert ((lo <= out["pos"]) & (out["pos"] < hi)).all()
    words = np.concatenate([u, np.array([0, 0xFF, 0x100, 0x7FFFFFFF, 0x80000000, 0x800000FF, 0xFFFFFF00, 0xFFFFFFFF],
                                        np.uint32), ctr[0]])
    got = dev("rng", u=words, lo=np.zeros(words.size, np.int32), hi=np.ones(words.size, np.int32))["action"]
    assert not nc.bit_differences(got, nc.np_u32_to_action(words)).size
    assert got.min() == -1.0 and got.max() == 1.0 - 2.0 ** -23


def _philox_per_element(ctr, key):
    """noise_ref.philox4x32's rounds with one key per element (uint64 arithmetic on uint32 words)"""
    c = [v.astype(np.uint64) for v in ctr]
    k0, k1 = (v.astype(np.uint64) for v in key)
    m32, s32 = np.uint64(noise_ref.U32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(noise_ref.M0) * c[0], np.uint64(noise_ref.M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k0, p1 & m32, (p0 >> s32) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(noise_ref.W0)) & m32, (k1 + np.uint64(noise_ref.W1)) & m32
    return np.stack(c).astype(np.uint32)


# ---------------------------------------------------------------- 3. through the engine
def test_observe_of_tiny_negative_rotations_equals_the_cpu_backend(oracle_mod):
    """`rot % 2` of a rotation in (-2^-53, 0) is 2.0 in Python (obs 9.8696), and of -0.0 it is 0.0: states no
    play reaches but load_state_dict accepts.  py_mod2_fast returned -5e-324 for -5e-324 (obs -0.0)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import skillshot_learning_amd as ssa
    n = 64
    ref = oracle_mod.OracleState(n, seed=7)
    ref.reset(random_positions=True)
    tiny = (-5e-324, -1e-323, -0.0, -1e-20)
    for k, v in enumerate(tiny):
        ref.rot[3 + 8 * k, 0] = v       # a player's rotation alone,
        ref.qrot[4 + 8 * k, 1] = v      # a projectile's alone,
        ref.rot[5 + 8 * k] = v          # and all four of a game
        ref.qrot[5 + 8 * k] = v
    ref.rot[40], ref.qrot[40] = (5e-324, 1e-20), (tiny[0], 0.0)
    games = {}
    for device in ("cuda", "cpu"):
        g = games[device] = ssa.VecSkillshotGame(n, device=device, seed=7)
        g.load_state_dict(ref.arrays())
        assert not nc.bit_differences(g.state_dict()["rot"], ref.rot).size  # the values survive the load
    obs = {d: g.observe()[0].cpu().numpy() for d, g in games.items()}
    for col in (4, 9):
        bad = nc.bit_differences(obs["cuda"][..., col], obs["cpu"][..., col])
        assert bad.size == 0, (col, bad[:5], obs["cuda"][..., col].ravel()[bad[:5]], obs["cpu"][..., col].ravel()[bad[:5]])
    want = np.float32(((2.0 * math.pi) / 2) * math.pi)  # `% 2 * np.pi) / 2 * np.pi` at 2.0
    assert obs["cuda"][0, 3, 4] == want and obs["cuda"][1, 4, 9] == want and obs["cuda"][0, 19, 4] == 0.0
    assert np.array_equal(obs["cuda"][:, 5, [4, 9]], np.full((2, 2), want))
    # get_state() of the same state: test_gpu_parity.test_features_match_oracle's rule, the rotations bit for bit
    f = games["cuda"].features().cpu().numpy()
    w = ref.features()
    exact = [1, 4, 5, 6, 7, 9, 11, 12, 13, 14, 15, 17]
    assert np.array_equal(f[..., exact], w[..., exact])
    assert not nc.bit_differences(f[..., [6, 13]], w[..., [6, 13]]).size
    err = np.abs(f - w) / np.maximum(1.0, np.abs(w))
    assert err.max() <= 1e-12, err.max()
