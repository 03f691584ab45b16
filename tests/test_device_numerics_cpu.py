"""The host twin of the numeric probes (oracle/sk_probe.hip built by g++ like
tests/trig_check.cpp) against the references the device is held to in
tests/test_device_numerics_gpu.py, the parity of the probe's device flag list
with the product's, the comparison helpers' own check, and the contents of the
shared input sets (tests/numerics_cases.py).

Bars (the project's own, reached through the probe's entry points):
  sincos_bf    <= 1 ulp from math.sin / math.cos (glibc, the reference's), exact at +-0
  sincos_fast  <= SKT_FAST_ERR / 2 from the correctly rounded sin / cos (tests/cr_tan.py)
  sincos_add   <= SKT_ADD_ERR / 2 from the correctly rounded sin / cos of the fp64 sum x + d
  ok           false exactly for |x| >= 2^20 * pi/2 and non-finite x
  tan_cr       == cr_tan bit for bit
  sincos_bf's s / c (grad_fast's quotient) within 2^-42 of cr_tan, relative: a quarter of kFutureMargin
"""
import math
import os
import re

import numpy as np
import pytest

import numerics_cases as nc
from cr_tan import cr_cos, cr_sin, cr_sincos, cr_tan
from oracle import probe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 20000


@pytest.fixture(scope="module")
def host_trig():
    """the twin over 20,000 angles: every edge value and an even draw of the sweeps"""
    rng = np.random.default_rng(11)
    full = nc.trig_inputs(N)
    m = full["x"].size
    n_edges = sum(len(v) for v in nc.edge_angles().values())  # the set's last elements
    pick = np.concatenate([rng.choice(m - n_edges, N - n_edges, replace=False), np.arange(m - n_edges, m)])
    inp = {k: v[pick].copy() for k, v in full.items()}
    inp["act"][0] = math.nan  # a NaN action on an angle inside the range
    assert abs(inp["x"][0]) < 1e6
    return inp, probe.run_host("trig", **inp)


def test_flag_lists_are_the_products():
    """the device probe is built with exactly skillshot_learning_amd/build.py's FLAGS, the twin with the host
    checks' g++ flags"""
    from skillshot_learning_amd import build
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    hip = re.search(r"^PROBE_HIPFLAGS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert hip == build.FLAGS
    recipe = re.search(r"^\t\$\(HIPCC\) (.*)$", mk, re.M).group(1).split()
    assert recipe == ["$(PROBE_HIPFLAGS)", "-o", "$@.tmp", "sk_probe.hip"]  # and nothing beside them
    host = re.search(r"^PROBE_HOSTFLAGS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    check = open(os.path.join(ROOT, "tests", "test_trig_cpu.py")).read()
    assert host == re.search(r'\["g\+\+", (.*?), "-o"', check).group(1).replace('"', "").split(", ")
    assert host == ["-O2", "-std=c++17", "-ffp-contract=off"]


def test_cr_sin_cos_against_mpmath():
    mp = pytest.importorskip("mpmath")
    mp.mp.prec = 400
    xs = nc.crafted_angles()
    xs = xs[np.isfinite(xs)]
    for x in list(xs) + [1e22]:
        s, c = cr_sincos(x)
        assert (s, c) == (float(mp.sin(mp.mpf(float(x)))), float(mp.cos(mp.mpf(float(x))))), repr(x)
    assert math.copysign(1.0, cr_sin(-0.0)) == -1.0 and cr_cos(-0.0) == 1.0
    assert cr_sin(5e-324) == 5e-324 and cr_tan(5e-324) == 5e-324


def test_twin_sincos_bf_within_one_ulp_of_glibc(host_trig):
    inp, out = host_trig
    x = inp["x"]
    ok = np.abs(x) < nc.FAST_MAX  # false for NaN
    assert np.array_equal(out["bf_ok"] != 0, ok) and np.array_equal(out["fast_ok"] != 0, ok)
    assert ok.sum() > 0.99 * N and (~ok).sum() >= 10
    xs = x[ok]
    us = nc.ulps(out["bf_s"][ok], np.array([math.sin(v) for v in xs]))
    uc = nc.ulps(out["bf_c"][ok], np.array([math.cos(v) for v in xs]))
    print(f"host twin sincos_bf: max {max(us.max(), uc.max()):.0f} ulp from glibc over {xs.size} angles")
    assert us.max() <= 1 and uc.max() <= 1
    zero = np.flatnonzero(x == 0)
    assert zero.size >= 2
    assert not nc.bit_differences(out["bf_s"][zero], x[zero]).size  # sin(+-0) = +-0
    assert not nc.bit_differences(out["bf_c"][zero], np.ones(zero.size)).size


def test_twin_sincos_fast_and_add_within_half_their_bounds(host_trig):
    inp, out = host_trig
    x, d = inp["x"], inp["d"].astype(np.float64)
    ok = out["fast_ok"] != 0
    ef = ea = 0.0
    for i in np.flatnonzero(ok):
        s, c = cr_sincos(x[i])
        ef = max(ef, abs(float(out["fast_s"][i]) - s), abs(float(out["fast_c"][i]) - c))
        s, c = cr_sincos(x[i] + d[i])  # the fp64 rotation after the look
        ea = max(ea, abs(float(out["add_s"][i]) - s), abs(float(out["add_c"][i]) - c))
    print(f"host twin: sincos_fast max error {ef:.3e}, sincos_add {ea:.3e}")
    assert ef <= nc.SKT_FAST_ERR / 2
    assert ea <= nc.SKT_ADD_ERR / 2


def test_twin_tan_cr_equals_the_decimal_tan():
    x = nc.angles(N)
    x = x[np.abs(x) < nc.TAN_CR_MAX]
    x = np.random.default_rng(12).choice(x, N, replace=False)
    x = np.concatenate([x, -nc.crafted_angles()[np.abs(nc.crafted_angles()) < 1e6] + math.pi / 2])
    got = probe.run_host("tan", x=x)["tan_cr"]
    want = np.array([cr_tan(v) for v in x])
    bad = nc.bit_differences(got, want)
    assert bad.size == 0, [(repr(x[i]), repr(got[i]), repr(want[i])) for i in bad[:5]]


def test_grad_quotient_inside_a_quarter_of_the_future_margin():
    """grad_fast's own arithmetic, sincos_bf(y) s / c at y = fl(-rot + pi/2), on the crafted rotations inside
    the fast range: relative error against cr_tan(y) at most 2^-42, so the inputs of the device test stay
    inside its bar by themselves"""
    rot = nc.crafted_angles()
    y = -rot + math.pi / 2
    y = y[np.abs(y) < nc.FAST_MAX]
    out = probe.run_host("trig", x=y)
    want = np.array([cr_tan(v) for v in y])
    with np.errstate(all="ignore"):
        g = out["bf_s"] / out["bf_c"]
    rel = nc.relative_error(g, want)
    print(f"host twin s / c: max relative error {rel.max():.3e} = 2^{math.log2(rel.max()):.1f} over {y.size}")
    assert nc.GRAD_BAR == nc.K_FUTURE_MARGIN / 4
    assert rel.max() <= nc.GRAD_BAR


def test_twin_range_predicates_equal_their_definitions():
    t = nc.range_tuples(1 << 16)
    got = nc.in_chunks(probe.run_host, "range", probe.MAX_ELEMENTS, v=t)["out"]
    want, defined = nc.range_definitions(t)
    assert set(np.unique(got)) <= {0, 1}
    bad = np.argwhere((got != want) & defined)
    assert bad.size == 0, [(probe.RANGE_PREDICATES[k], t[:, i].tolist()) for k, i in bad[:5]]
    for k, name in enumerate(probe.RANGE_PREDICATES):  # both answers occur where the definition applies
        assert set(np.unique(want[k][defined[k]])) == {0, 1}, name


def test_comparison_helpers_report_single_element_changes(host_trig):
    inp, out = host_trig
    assert nc.twin_differences("trig", inp, out, out) == []
    i = int(np.flatnonzero(out["bf_ok"] != 0)[100])
    # one ulp in one element
    other = {k: v.copy() for k, v in out.items()}
    other["bf_s"][i] = np.nextafter(out["bf_s"][i], 2.0)
    assert nc.twin_differences("trig", inp, other, out) == [("bf_s", i)]
    assert nc.ulps(other["bf_s"], out["bf_s"])[i] == 1
    other = {k: v.copy() for k, v in out.items()}
    other["fast_c"][i] = np.nextafter(out["fast_c"][i], np.float32(2))
    assert nc.twin_differences("trig", inp, other, out) == [("fast_c", i)]
    # one flipped flag (an ok bit outside the compared values' range too)
    for name in nc.TRIG_FLAGS:
        for j in (i, int(np.flatnonzero(out["bf_ok"] == 0)[0])):
            other = {k: v.copy() for k, v in out.items()}
            other[name][j] ^= 1
            assert (name, j) in nc.twin_differences("trig", inp, other, out)
    # a NaN's payload and its sign
    j = int(np.flatnonzero(np.isnan(out["move_x"]) & (out["fast_ok"] != 0))[0])
    for flip in (np.uint32(1), np.uint32(0x80000000)):
        other = {k: v.copy() for k, v in out.items()}
        other["move_x"].view(np.uint32)[j] ^= flip
        assert np.isnan(other["move_x"][j])
        assert nc.twin_differences("trig", inp, other, out) == [("move_x", j)]
    # -0.0 against 0.0, and the tan group's range
    z = np.array([0.0, 1.0]), np.array([-0.0, 1.0])
    assert nc.bit_differences(*z).tolist() == [0] and nc.bit_differences(z[0], z[0]).size == 0
    x = np.array([1.0, 2.0 ** 20])
    a, b = dict(tan_cr=np.array([1.5, 7.0])), dict(tan_cr=np.array([np.nextafter(1.5, 2), 8.0]))
    assert nc.twin_differences("tan", dict(x=x), a, b) == [("tan_cr", 0)]


def test_input_sets_contain_every_named_edge():
    a, c = nc.angles(N), nc.crafted_angles()
    for name, values in nc.edge_angles().items():
        for s in (a, c):
            have = set(nc.bits(s).tolist())
            assert all(int(nc.bits(np.float64(v).reshape(1))[0]) in have for v in values), name
    for v in (0.0, -0.0, nc.FAST_MAX, np.nextafter(nc.FAST_MAX, 0), np.nextafter(nc.FAST_MAX, 1e9), 2.0 ** 40,
              2.0 ** 40 + 0.25, 1e8, 1e15, 5e-324, -5e-324, math.inf, -math.inf, math.pi / 4, -100 * math.pi,
              np.nextafter(math.pi / 2, 0), -10.0, 0.25):
        assert int(nc.bits(np.float64(v).reshape(1))[0]) in set(nc.bits(a).tolist()), v
    assert np.isnan(a).any() and np.isnan(c).any() and c.size <= 2048
    la = nc.lib_angles(1 << 12)
    assert np.abs(la).min() >= nc.FAST_MAX and np.abs(la).max() == 1e15 and (la < 0).any()
    m = nc.mod2_values()
    have = set(nc.bits(m).tolist())
    for name, values in nc.mod2_edges().items():
        assert all(int(nc.bits(np.float64(v).reshape(1))[0]) in have for v in values), name
    for v in (-5e-324, 5e-324, -1e-323, -0.0, 0.0, -1e-20, 1e-20, 100.0, -100.0, np.nextafter(2.0, 3), 2.0 ** 53,
              -(2.0 ** 52) - 1, -1.7976931348623157e308, math.inf):
        assert int(nc.bits(np.float64(v).reshape(1))[0]) in have, v
    mags = np.log10(np.abs(m[np.isfinite(m) & (m != 0)]))
    assert np.histogram(mags, bins=60, range=(-30, 30))[0].min() > 0  # 60 decades
    want = nc.py_mod2(np.array([-5e-324, -1e-323, -0.0, -1e-20, 3.5, -3.5, math.inf]))
    assert want[:6].tolist() == [2.0, 2.0, 0.0, 2.0, 1.5, 0.5] and math.isnan(want[6])
    assert math.copysign(1, want[2]) == 1
    p = nc.dist_points(1 << 10).astype(np.int64)
    d = {(abs(ax - bx), abs(ay - by)) for ax, ay, bx, by in p.T.tolist()}
    assert {(i, j) for i in range(251) for j in range(251)} <= d
    assert (1 << 20, 1 << 20) in d and (46341, 46341) in d and p.max() == 1 << 20
    g, _ = nc.line_points()
    assert (np.abs(g - 1.0) < 1e-15).any() and (np.abs(g + 1.0) < 1e-15).any()  # math.tan(pi/4) is 1 - 2^-53
    assert (g == 0.0).any() and (np.abs(g) > 1.6e16).any() and np.isnan(g).any()
    t = nc.range_tuples(1 << 10)
    for v in (32767, 32768, 65535, 65536, 65537, -1, -256, 255, 256, nc.BIG, nc.BIG + 1):
        assert (t[0] == v).any(), v
    ctr, key = nc.rng_words(16)
    w = np.concatenate([ctr, key])
    assert {tuple(col) for col in (w[:, :64] != 0).T.tolist()} == {tuple(map(bool, f)) for f in np.ndindex(*[2] * 6)}
    u, lo, hi = nc.pos_draws(16)
    assert (25, 225) in nc.rand_ranges() and len(nc.rand_ranges()) >= 4
    for a_lo, a_hi in nc.rand_ranges():
        sel = (lo == a_lo) & (hi == a_hi)
        pos = nc.np_u32_to_pos(u[sel], lo[sel], hi[sel])
        assert set(pos.tolist()) == set(range(a_lo, a_hi))  # every bucket, none outside
        assert {0, 0xFFFFFFFF} <= set(u[sel].tolist())
        us = np.sort(u[sel].astype(np.int64))
        edge = np.flatnonzero(np.diff(nc.np_u32_to_pos(us.astype(np.uint32), lo[sel], hi[sel])) != 0)
        assert edge.size == a_hi - a_lo - 1 and (us[edge + 1] - us[edge] == 1).all()  # both sides of every edge
