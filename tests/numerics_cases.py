"""Inputs, references and comparison helpers shared by
tests/test_device_numerics_cpu.py and tests/test_device_numerics_gpu.py: the
numeric primitives of the step engine (csrc/sk_trig.hpp, sk_tan_cr.hpp,
sk_range.hpp and the device-only helpers of sk_device.hpp), evaluated element
by element through the probes (oracle/sk_probe.hip, oracle/probe.py).

Every set is deterministic from its seed.  Nothing here runs a kernel.
"""
import functools
import math
from decimal import Decimal, localcontext

import numpy as np

FAST_MAX = 1647099.3291652855  # sktrig::sincos_bf's / sincos_fast's range, 2^20 * pi/2
TAN_CR_MAX = 1048576.0         # sktan::tan_cr hands |x| >= 2^20 to the platform's tan
SKT_FAST_ERR = float(np.float32(3.0e-7))
SKT_ADD_ERR = float(np.float32(6.0e-7))
K_FUTURE_MARGIN = 2.0 ** -40   # sk_device.hpp kFutureMargin
GRAD_BAR = 2.0 ** -42          # the gradient's relative error must stay a factor 4 inside it
PI4 = math.pi / 4
SPEEDS = (3.0, 5.0, 4.0, 6.0, 11.0, 23.0)  # the player / projectile speeds of the small-board configurations
SUBNORMALS = (5e-324, 1e-323, 1.5e-323, 2e-323, 2.5e-323, 1e-310, 2.2250738585072009e-308)


def _frozen(a):
    a.setflags(write=False)
    return a


def _both_signs(v):
    v = np.asarray(v, np.float64)
    return np.concatenate([v, -v])


# ---------------------------------------------------------------- angles
def tie_rotations(speed):
    """tests/test_multi_fast_trig_gpu.py's _tie_rotations: rotations whose sine or cosine times `speed` is a
    half-integer, their neighbours, and the probes 1e-9 and 1e-6 away"""
    out = []
    for k in range(1, 2 * speed, 2):
        for r0 in (math.asin(k / (2.0 * speed)), math.acos(k / (2.0 * speed))):
            out += [r0, np.nextafter(r0, 10.0), np.nextafter(r0, -10.0), r0 + 1e-9, r0 - 1e-9, r0 + 1e-6, r0 - 1e-6]
    return [float(r) for r in out]


def edge_angles():
    """name -> the named edge values of the angle sets (every one is in `angles` and in `crafted_angles`)"""
    return dict(
        zeros=[0.0, -0.0],
        range_edge=[FAST_MAX, float(np.nextafter(FAST_MAX, 0.0)), float(np.nextafter(FAST_MAX, math.inf)),
                    -FAST_MAX, -float(np.nextafter(FAST_MAX, 0.0)), -float(np.nextafter(FAST_MAX, math.inf))],
        large=[2.0 ** 40, 2.0 ** 40 + 0.25, 1e8, 1e15, -(2.0 ** 40), -(2.0 ** 40 + 0.25), -1e8, -1e15],
        subnormal=[s * v for v in SUBNORMALS for s in (1.0, -1.0)],
        nonfinite=[math.nan, math.inf, -math.inf],
        ties=tie_rotations(3) + tie_rotations(5),
    )


def _pi4_neighbours(kmax, offsets):
    c = np.arange(-kmax, kmax + 1) * PI4
    return np.concatenate([c + o for o in offsets] + [np.nextafter(c, 1e9), np.nextafter(c, -1e9)])


@functools.lru_cache(maxsize=None)
def angles(n, seed=0):
    """the sweeps of tests/trig_check.cpp and tests/test_tan_cr_cpu.py with n random values in the main sweep,
    and every edge value"""
    rng = np.random.default_rng(seed)
    grid = 0.25 * rng.integers(0, 4001, n // 4) - 500.0 + 0.25 * rng.uniform(-1, 1, n // 4)
    k64 = np.arange(-64, 65) * PI4
    parts = [
        rng.uniform(-600.0, 600.0, n), rng.uniform(-4.0, 4.0, n // 4), rng.uniform(-1.6e6, 1.6e6, n // 4),
        _pi4_neighbours(400, [j * 1e-9 for j in range(-3, 4)]), grid,
        # test_tan_cr_cpu.py's rotations
        rng.uniform(-math.pi, math.pi, n // 4), rng.uniform(-60, 60, n // 4), rng.uniform(-1000, 1000, n // 8),
        k64, k64 + rng.choice([-1e-15, 1e-15, -1e-12, 1e-9], k64.size), np.arange(-40, 41) * 0.25,
        rng.uniform(-1e-6, 1e-6, 64),
    ] + [np.array(v) for v in edge_angles().values()]
    return _frozen(np.concatenate(parts).astype(np.float64))


@functools.lru_cache(maxsize=None)
def crafted_angles(seed=1):
    """at most 2,048 angles for the comparisons with the Decimal reference: every edge value, the multiples of
    pi/4 that give gradients 0, +-1 and ~1.6e16 with their neighbours, the look grid, a few of each sweep"""
    rng = np.random.default_rng(seed)
    parts = [_pi4_neighbours(64, [0.0, 1e-9, -1e-9]), np.arange(-40, 41) * 0.25,
             rng.uniform(-600.0, 600.0, 400), rng.uniform(-4.0, 4.0, 150), rng.uniform(-1.6e6, 1.6e6, 400),
             rng.uniform(-1e-6, 1e-6, 16)] + [np.array(v) for v in edge_angles().values()]
    a = np.concatenate(parts).astype(np.float64)
    assert a.size <= 2048, a.size
    return _frozen(a)


@functools.lru_cache(maxsize=None)
def lib_angles(n, seed=2):
    """arguments past the fast range, 1.6e6 .. 1e15 in magnitude: log-uniform, quarter-step look grids on large
    rotations, doubles next to multiples of pi/2, and the large edge values"""
    rng = np.random.default_rng(seed)
    mag = np.exp(rng.uniform(math.log(FAST_MAX), math.log(1e15), n))
    k = rng.integers(2 ** 20 + 1, 2 ** 48, n // 8).astype(np.float64)
    e = edge_angles()
    parts = [mag * rng.choice([-1.0, 1.0], n), k * (math.pi / 2), -k * (math.pi / 2),
             2.0 ** 40 + 0.25 * rng.integers(-4000, 4000, n // 8),
             np.array([v for v in e["range_edge"] if abs(v) >= FAST_MAX]), np.array(e["large"])]
    return _frozen(np.concatenate(parts).astype(np.float64))


@functools.lru_cache(maxsize=None)
def trig_inputs(n, seed=3):
    """the trig group's inputs over `angles(n)`: look steps d = a * 0.25 as the fast tick forms them (with the
    ends of sincos_add's range), speeds, clamped move actions (ties, +-1, NaN), round_safe pairs next to
    half-integers, look speeds on both sides of look_fits_add's bound"""
    rng = np.random.default_rng(seed)
    x = angles(n)
    m = x.size

    def cycle(edges, rand):
        a = np.asarray(rand, np.float32).copy()
        e = np.asarray(edges, np.float32)
        a[:e.size] = e
        return rng.permutation(a)

    f32 = np.float32
    d = cycle([0.0, -0.0, 0.25, -0.25, PI4, -PI4, 1e-8, -1e-8],
              rng.uniform(-1, 1, m).astype(f32) * f32(0.25))
    speed = rng.choice(np.array(SPEEDS, f32), m)
    act = cycle([1.0, -1.0, 0.0, -0.0, 0.5 / 3, -0.5 / 3, 0.5 / 5, math.nan, 1e-30, np.nextafter(f32(1), f32(0))],
                rng.uniform(-1, 1, m))
    half = rng.integers(-30, 30, m) + 0.5
    rs_d = cycle([0.5, -0.5, 1.5, 2.5, 0.0, math.nan, math.inf, -math.inf, 8388608.5, 1e30],
                 half + rng.choice([0.0, 1e-6, -1e-6, 3e-6, -3e-6, 1e-5, 0.25, -0.4], m))
    rs_eps = rng.choice(np.array([1e-6 * s for s in SPEEDS] + [2e-6 * s for s in SPEEDS], f32), m)
    look = rng.uniform(-1.0, 1.0, m)
    le = _both_signs([PI4, np.nextafter(PI4, 0.0), np.nextafter(PI4, 1.0), 0.25, 0.4, 0.8, 3.0, 0.0, math.inf])
    look[:le.size] = le
    look[le.size] = math.nan
    return dict(x=x, d=_frozen(d), speed=_frozen(speed), act=_frozen(act), rs_d=_frozen(rs_d),
                rs_eps=_frozen(rs_eps), look=_frozen(rng.permutation(look)))


@functools.lru_cache(maxsize=None)
def random_trig_inputs(n=1 << 20, seed=13):
    """n random elements of every trig input: half the angles over the game's rotations, a quarter over and just
    past the fast range, a quarter random bit patterns (every exponent, NaNs with payloads)"""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    x = np.concatenate([rng.uniform(-600.0, 600.0, n // 2), rng.uniform(-1.7e6, 1.7e6, n // 4),
                        rng.integers(0, 1 << 64, n - n // 2 - n // 4, dtype=np.uint64).view(np.float64)])
    return dict(x=_frozen(x), d=_frozen(rng.uniform(-1, 1, n).astype(f32) * f32(0.25)),
                speed=_frozen(rng.choice(np.array(SPEEDS, f32), n)), act=_frozen(rng.uniform(-1, 1, n).astype(f32)),
                rs_d=_frozen(rng.uniform(-120, 120, n).astype(f32)),
                rs_eps=_frozen(rng.choice(np.array([1e-6 * s for s in SPEEDS] + [2e-6 * s for s in SPEEDS], f32), n)),
                look=_frozen(rng.uniform(-2, 2, n)))


@functools.lru_cache(maxsize=None)
def crafted_reference():
    """the Decimal references over crafted_angles(), computed once: sin, cos, tan of x and the gradient
    tan(fl(-x + pi/2)), NaN where x is not finite"""
    from cr_tan import cr_sincos, cr_tan
    x = crafted_angles()
    ref = {k: np.full(x.size, math.nan) for k in ("sin", "cos", "tan", "grad")}
    for i, v in enumerate(x.tolist()):
        if math.isfinite(v):
            ref["sin"][i], ref["cos"][i] = cr_sincos(v)
            ref["tan"][i] = cr_tan(v)
            ref["grad"][i] = cr_tan(-v + math.pi / 2)
    return {k: _frozen(v) for k, v in ref.items()}


def relative_error(got, want):
    """|got - want| / |want|, 0 where they are equal (0 against 0), inf where one is NaN and the other not"""
    with np.errstate(all="ignore"):
        rel = np.abs(got - want) / np.abs(want)
    rel[got == want] = 0.0
    rel[np.isnan(got) != np.isnan(want)] = np.inf
    return rel


# ---------------------------------------------------------------- py_mod2
def mod2_edges():
    even = np.arange(-100, 101, 2, dtype=np.float64)
    return dict(
        zeros=[0.0, -0.0],
        subnormal=[s * v for v in SUBNORMALS for s in (1.0, -1.0)],
        tiny=[1e-20, -1e-20],
        even=np.concatenate([even, np.nextafter(even, math.inf), np.nextafter(even, -math.inf)]).tolist(),
        big=[s * v for v in (2.0 ** 52 - 1, 2.0 ** 52, 2.0 ** 52 + 1, 2.0 ** 53, 1.7976931348623157e308)
             for s in (1.0, -1.0)],
        nonfinite=[math.nan, math.inf, -math.inf],
    )


@functools.lru_cache(maxsize=None)
def mod2_values(n=1 << 16, seed=4):
    rng = np.random.default_rng(seed)
    rand = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-30, 30, n)  # 60 decades
    parts = [np.array(v, np.float64) for v in mod2_edges().values()] + [rand, rng.uniform(-600, 600, n)]
    return _frozen(np.concatenate(parts))


def py_mod2(values):
    """Python's r % 2 element by element (NaN for NaN and +-inf, where Python gives NaN or raises)"""
    return np.array([float(r) % 2.0 if math.isfinite(r) else math.nan for r in values], np.float64)


# ---------------------------------------------------------------- distances
@functools.lru_cache(maxsize=None)
def dist_points(n=1 << 16, seed=5):
    """int32 [4, m] (ax, ay, bx, by): every pair of differences in 0..250 (signs varied), differences up to 2^20
    (what sk_config admits) with the values around 46,340 where an int sum of squares wraps"""
    rng = np.random.default_rng(seed)
    dx, dy = (v.ravel() for v in np.meshgrid(np.arange(251), np.arange(251), indexing="ij"))
    sx, sy = rng.choice([-1, 1], dx.size), rng.choice([-1, 1], dx.size)
    bx, by = rng.integers(0, 251, dx.size), rng.integers(0, 251, dx.size)
    small = np.stack([bx + sx * dx, by + sy * dy, bx, by])
    edge = np.array([0, 1, 46340, 46341, 65535, 65536, (1 << 20) - 1, 1 << 20])
    ex, ey = (v.ravel() for v in np.meshgrid(edge, edge, indexing="ij"))
    big_dx = np.concatenate([ex, rng.integers(0, (1 << 20) + 1, n)])
    big_dy = np.concatenate([ey, rng.integers(0, (1 << 20) + 1, n)])
    flip = rng.choice([False, True], big_dx.size)
    zero = np.zeros_like(big_dx)
    big = np.stack([np.where(flip, zero, big_dx), np.where(flip, big_dy, zero), np.where(flip, big_dx, zero),
                    np.where(flip, zero, big_dy)])
    return _frozen(np.concatenate([small, big], axis=1).astype(np.int32))


def cr_dist_point_point(p):
    """the correctly rounded sqrt of the exact integer sum of squares (Python ints, rounded through Decimal: an
    integer's root is exact or irrational, farther than 1e-39 from any fp64 rounding midpoint here)"""
    out = np.empty(p.shape[1], np.float64)
    with localcontext() as ctx:
        ctx.prec = 60
        for i, (ax, ay, bx, by) in enumerate(p.T.tolist()):
            out[i] = float(Decimal((ax - bx) ** 2 + (ay - by) ** 2).sqrt())
    return out


@functools.lru_cache(maxsize=None)
def line_points(seed=6):
    """(g f64 [m], p int32 [4, m]): gradients math.tan(-r + pi/2) over the crafted angles (0, +-1, ~1.6e16,
    NaN for the non-finite ones), each with several point pairs on the reference's board and on a huge one"""
    rng = np.random.default_rng(seed)
    r = np.repeat(crafted_angles(), 8)
    g = np.array([math.tan(-v + math.pi / 2) if math.isfinite(v) else math.nan for v in r])
    hi = np.where(rng.random(r.size) < 0.75, 251, (1 << 20) + 1)
    p = rng.integers(0, hi, (4, r.size))
    return _frozen(g), _frozen(p.astype(np.int32))


def np_dist_line_point(g, p):
    """SkillshotGame.get_dist_line_point in numpy fp64, one rounding per operation, the reference's order"""
    lx, ly, cx, cy = (v.astype(np.float64) for v in p)
    with np.errstate(all="ignore"):
        cc = ly - g * lx
        return np.abs(g * cx - cy + cc) / np.sqrt(g * g + 1.0)


@functools.lru_cache(maxsize=None)
def clamp_values(n=4096, seed=7):
    rng = np.random.default_rng(seed)
    e = _both_signs([0.0, 1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), 1.5, math.inf, 5e-324, 0.5])
    a = np.concatenate([e, [math.nan], rng.uniform(-2, 2, n)])
    f32 = np.float32
    ef = _both_signs([0.0, 1.0, 1.5, math.inf, 0.5]).astype(f32)
    nf = np.array([np.nextafter(f32(1), f32(0)), np.nextafter(f32(1), f32(2)), -np.nextafter(f32(1), f32(0)),
                   -np.nextafter(f32(1), f32(2)), f32(math.nan), f32(1e-45)], f32)
    af = np.concatenate([ef, nf, rng.uniform(-2, 2, a.size - ef.size - nf.size).astype(f32)])
    return _frozen(a), _frozen(af)


def clamp(a):
    """Player.py:36-37, :60-61: `1 if a >= 1 else a`, then `-1 if a <= -1 else a` (a NaN passes through)"""
    one = a.dtype.type(1)
    a = np.where(a >= one, one, a)
    return np.where(a <= -one, -one, a)


# ---------------------------------------------------------------- range predicates
def _grid(*lists):
    return np.stack([v.ravel() for v in np.meshgrid(*[np.asarray(l, np.int64) for l in lists], indexing="ij")])


def _pad8(t):
    out = np.zeros((8, t.shape[1]), np.int64)
    out[:t.shape[0]] = t
    return out


BIG = 1 << 20
WRAP_VALUES = (-BIG - 1, -BIG, -70000, -65537, -65536, -32769, -32768, -257, -256, -2, -1, 0, 1, 2, 127, 128, 254,
               255, 256, 257, 32767, 32768, 32769, 65534, 65535, 65536, 65537, 70000, BIG - 1, BIG, BIG + 1)


@functools.lru_cache(maxsize=None)
def range_tuples(n_random=1 << 20, seed=8):
    """int32 [8, m]: the sweeps of tests/pair_collision_check.cpp and tests/steady_admit_check.cpp as arrays
    (every predicate reads the leading values of each tuple), boundary values plus and minus one, negative
    values, values at and past 2^15 and 2^16 where an unsigned compare wraps; then n_random random tuples"""
    rng = np.random.default_rng(seed)
    parts = []
    # fits_axis (n, room), fits_board (nx, ny, room_x, room_y)
    rooms = [0, 1, 2, 5, 245, 247, 255, 293, 32767, 32768, 65535, 65536, BIG - 1, BIG, -1, -5]
    for room in rooms:
        near = [room - 1, room, room + 1]
        parts.append(_pad8(_grid(list(WRAP_VALUES) + near, [room])))
        parts.append(_pad8(_grid([-1, 0, 1] + near, [-1, 0, 1] + near, [room], [room, 245, 0])))
    # check_bounds: a board position minus every step
    for W, H, ps, qs in ((250, 250, 5, 3), (250, 250, 1, 1), (255, 255, 255, 255), (300, 7, 7, 2)):
        p = np.arange(-2, W + 3)
        steps = np.concatenate([np.arange(-300, 301), [-BIG, -70000, -256, 256, 70000, BIG]])
        npos = np.unique(p[:, None] - steps[None, :])  # each distinct position once
        for size in (ps, qs):
            for o in (-1, 0, 1):
                other = np.full_like(npos, H - size + o)
                parts.append(_pad8(np.stack([npos, other, np.full_like(npos, W - size), np.full_like(npos, H - size)])))
                parts.append(_pad8(np.stack([other, npos, np.full_like(npos, H - size), np.full_like(npos, W - size)])))
    # box_hit (px, py, psize, oqx, oqy, qsize): check_intervals
    pq = _grid(np.arange(256), np.arange(256))
    p, q = pq[0], pq[1]
    c100 = np.full_like(p, 100)
    for k, (ps, qs) in enumerate(((5, 3), (1, 1), (255, 255), (1, 255), (255, 1))):
        s, t = np.full_like(p, ps), np.full_like(p, qs)
        parts.append(_pad8(np.stack([p, 255 - p, s, q, 255 - q, t])))
        if k == 0:
            parts.append(_pad8(np.stack([p, c100, s, q, c100, t])))
            parts.append(_pad8(np.stack([c100, p, s, c100, q, t])))
    parts.append(_pad8(_grid([0, 100, -3], [50], [0, 5, -1, 65535, 65536], WRAP_VALUES, [50, 47, 56], [3, 0, -2])))
    # pair_hit (lv, hit_p1, hit_p2): nonzero means true
    parts.append(_pad8(_grid([0, 1, 2, -1], [0, 1, 7], [0, 1, -4])))
    # pack_fits_player / admit_player (px, py, qx, qy, cd, age, qv): steady_admit_check's entries and one past
    cds = [-129, -128, -127, -1, 0, 1, 5, 15, 126, 127, 128]
    ages = [-1, 0, 1, 128, 240, 250, 251, 254, 255, 256]
    for pos in ((0, 0, 0, 0), (255, 255, 255, 255), (256, 0, 0, 0), (0, -1, 0, 0), (0, 0, 256, 0), (0, 0, 0, -1),
                (65536, 0, 0, 0), (0, 0, 0, 65536 + 7)):
        parts.append(_pad8(_grid(*[[v] for v in pos], cds, ages, [-1, 0, 1, 2])))
    full = _grid(np.arange(-128, 128), np.arange(0, 256), [1])  # every (qcd, qage) entry
    parts.append(_pad8(np.concatenate([np.zeros((4, full.shape[1]), np.int64), full])))
    # pack_fits_game (ticks, live, winner) / admit_game (ticks, live, winner, left)
    parts.append(_pad8(_grid([-1, 0, 1, 65523, 65524, 65534, 65535, 65536, 65537, BIG], [-1, 0, 1, 2],
                             [-1, 0, 1, 2, 3, 4], [-1, 0, 1, 2, 10, 12, 399, 400, 65534, 65535, 65536, 65537, BIG])))
    # cfg_ok (W, H, psize, qsize, pspeed, qspeed) / admit_cfg (W, H, psize, qsize, cdmax)
    sides = [1, 2, 4, 250, 255, 260, 261, BIG - 1, BIG, BIG + 1, 1 << 21]
    sizes = [-1, 0, 1, 3, 4, 5, 250, 255, 256]
    parts.append(_pad8(_grid([250, 4, 260, 261, BIG, BIG + 1], [250, 2, 260, 261], [5, 4, -1, 0, 255], [3, 5, 4, -1, 0],
                             [-1, 0, 3, 15, 127, 128, -BIG - 1, -BIG, BIG, BIG + 1], [5, -BIG - 1, BIG, 1 << 21])))
    m = 1 << 15
    parts.append(_pad8(np.stack([rng.choice(sides, m), rng.choice(sides, m), rng.choice(sizes, m),
                                 rng.choice(sizes, m), rng.choice([-BIG - 1, -BIG, -1, 0, 3, 127, 128, BIG, BIG + 1], m),
                                 rng.choice([-BIG - 1, -BIG, 5, BIG, BIG + 1], m)])))
    # random tuples: board-sized, byte-sized around the edges, and wide
    k = n_random // 4
    parts += [rng.integers(-40, 300, (8, k)), rng.integers(-2, 258, (8, k)), rng.integers(-(1 << 22), 1 << 22, (8, k)),
              rng.choice(np.array(WRAP_VALUES), (8, n_random - 3 * k))]
    t = np.concatenate(parts, axis=1)
    assert np.abs(t).max() <= 1 << 22  # sums of three stay inside int
    return _frozen(t.astype(np.int32))


def range_definitions(t):
    """-> (want uint8 [11, m], defined bool [11, m]) in oracle.probe.RANGE_PREDICATES' order: each predicate as
    its plain two-sided inequalities on Python-sized integers.  `defined`: sk_range.hpp's precondition for the
    one-compare form (hi >= lo), which the host checks for every configuration that runs it."""
    v = t.astype(np.int64)
    a, b, c, d, e, f, g = v[:7]
    yes = np.ones(t.shape[1], bool)

    def within(x, lo, hi):
        return (lo <= x) & (x <= hi)

    cfg_ok = ((a <= BIG) & (b <= BIG) & (c >= 0) & (d >= 0) & (c <= a) & (c <= b) & (d <= a) & (d <= b) &
              within(e, -BIG, BIG) & within(f, -BIG, BIG))
    fits_axis = within(a, 0, b)
    fits_board = within(a, 0, c) & within(b, 0, d)
    # (px, py, psize, oqx, oqy, qsize): hit_test_s of sk_device.hpp without its validity flag
    L, R, T, B = a, a + c, b, b + c
    ql, qr, qt, qb = d, d + f, e, e - f
    box_hit = (within(qr, L, R) | within(ql, L, R)) & (within(qt, T, B) | within(qb, T, B))
    lv, h1, h2 = a != 0, b != 0, c != 0
    pair_h1 = lv & h1
    pair_h2 = lv & ~pair_h1 & h2
    byte = [within(x, 0, 255) for x in (a, b, c, d)]
    pfp = byte[0] & byte[1] & byte[2] & byte[3] & within(e, -128, 127) & within(f, 0, 255) & within(g, 0, 1)
    pfg = within(a, 0, 65535) & within(b, 0, 1) & within(c, 0, 3)
    admit_cfg = within(e, 0, 127) & (a - c <= 255) & (b - c <= 255) & (a - d <= 255) & (b - d <= 255)
    admit_player = pfp & (f + np.maximum(e, 0) <= 255)
    admit_game = pfg & within(d, 0, 65535) & (a + d <= 65535)
    want = np.stack([cfg_ok, fits_axis, fits_board, box_hit, pair_h1, pair_h2, pfp, pfg, admit_cfg, admit_player,
                     admit_game]).astype(np.uint8)
    defined = np.stack([yes, b >= 0, (c >= 0) & (d >= 0), c >= 0, yes, yes, yes, yes, yes, yes, yes])
    return want, defined


# ---------------------------------------------------------------- rng
@functools.lru_cache(maxsize=None)
def rng_words(n=1 << 16, seed=9):
    """(ctr uint32 [4, m], key uint32 [2, m]): counters and keys at 0 and all-ones in every combination, then
    random 32-bit words"""
    rng = np.random.default_rng(seed)
    ends = _grid(*[[0, 0xFFFFFFFF]] * 6)
    w = np.concatenate([ends, rng.integers(0, 1 << 32, (6, n))], axis=1).astype(np.uint32)
    return _frozen(w[:4].copy()), _frozen(w[4:].copy())


def rand_ranges():
    """every (rand_lo, rand_hi) of the default configuration and of tests/config_cases.py's"""
    import config_cases as cc
    import golden_replay as gr
    cfgs = [gr.CFG_DEFAULT] + [cc.cfg_dict(name) for name in cc.NAMES]
    return sorted({(int(c["rand_lo"]), int(c["rand_hi"])) for c in cfgs})


@functools.lru_cache(maxsize=None)
def pos_draws(n_random=4096, seed=10):
    """(u uint32, lo int32, hi int32): for every random-start range u = 0, 2^32 - 1, the first word of every
    bucket and the last of the one before, and random words"""
    rng = np.random.default_rng(seed)
    us, los, his = [], [], []
    for lo, hi in rand_ranges():
        span = hi - lo
        first = [-((-j << 32) // span) for j in range(1, span)]  # ceil(j * 2^32 / span)
        u = np.array([0, 0xFFFFFFFF] + first + [x - 1 for x in first], np.uint64)
        u = np.concatenate([u, rng.integers(0, 1 << 32, n_random, dtype=np.uint64)])
        us.append(u)
        los.append(np.full(u.size, lo))
        his.append(np.full(u.size, hi))
    return (_frozen(np.concatenate(us).astype(np.uint32)), _frozen(np.concatenate(los).astype(np.int32)),
            _frozen(np.concatenate(his).astype(np.int32)))


def np_u32_to_action(u):
    """uniform [-1, 1): ((u >> 8) - 2^23) * 2^-23, exact in fp32"""
    return ((u.astype(np.int64) >> 8) - 8388608).astype(np.float32) * np.float32(2.0 ** -23)


def np_u32_to_pos(u, lo, hi):
    span = (hi.astype(np.int64) - lo).astype(np.uint64)
    return (lo.astype(np.int64) + ((u.astype(np.uint64) * span) >> np.uint64(32)).astype(np.int64)).astype(np.int32)


# ---------------------------------------------------------------- comparisons
def bits(a):
    """the bit patterns of an array, as unsigned integers of its item size"""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def bit_differences(got, want, where=None):
    """indices (into the flattened arrays) whose bit patterns differ -- NaNs by payload and sign, -0.0 != 0.0 --
    among the elements `where` selects"""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    diff = bits(got).ravel() != bits(want).ravel()
    if where is not None:
        diff &= np.broadcast_to(where, got.shape).ravel()
    return np.flatnonzero(diff)


def ulps(a, b):
    """distance in units of the last place between fp64 arrays (the ordered-integer distance; NaN -> huge)"""
    def key(x):
        i = np.ascontiguousarray(x, np.float64).view(np.int64)
        return np.where(i < 0, np.int64(-2 ** 63) - i, i)
    d = np.abs(key(a).astype(object) - key(b).astype(object)).astype(np.float64)
    return np.where(np.isnan(a) | np.isnan(b), np.inf, d)


# which outputs of the trig and tan groups are compared where: sincos_bf's values are declared meaningless
# (and its (int)fn is undefined) where ok is false; sincos_fast's are taken through inf - inf there, whose NaN
# an x86 host and the device sign differently, and everything derived from it alike; tan_cr calls the
# platform's tan from 2^20.  The flags are compared everywhere.
TRIG_VALUES = dict(bf_s="bf_ok", bf_c="bf_ok", fast_s="fast_ok", fast_c="fast_ok", add_s="fast_ok", add_c="fast_ok",
                   move_x="fast_ok", move_y="fast_ok", step_x="fast_ok", step_y="fast_ok")
TRIG_FLAGS = ("bf_ok", "fast_ok", "rs", "move_safe", "step_safe", "look_fits")


def twin_differences(group, inputs, got, want):
    """[(output name, element index)] where a probe's result `got` differs bit for bit from the twin's `want`"""
    out = []
    if group == "trig":
        for name in TRIG_FLAGS:
            out += [(name, int(i)) for i in bit_differences(got[name], want[name])]
        for name, flag in TRIG_VALUES.items():
            out += [(name, int(i)) for i in bit_differences(got[name], want[name], want[flag] != 0)]
    elif group == "tan":
        inside = np.abs(inputs["x"]) < TAN_CR_MAX
        out += [("tan_cr", int(i)) for i in bit_differences(got["tan_cr"], want["tan_cr"], inside)]
    else:
        for name in want:
            out += [(name, int(i)) for i in bit_differences(got[name], want[name])]
    return out


def in_chunks(run, group, chunk, **inputs):
    """run(group, **inputs) in launches of at most `chunk` elements, results concatenated"""
    n = next(iter(inputs.values())).shape[-1]
    outs = [run(group, **{k: np.ascontiguousarray(v[..., i:i + chunk]) for k, v in inputs.items()})
            for i in range(0, n, chunk)]
    return {k: np.concatenate([o[k] for o in outs], axis=-1) for k in outs[0]}
