"""The fp32-trig form of the step-only split tick (SK_MULTI_SPLIT=1 with
SK_MULTI_FAST=1: k_step_split_multi's FAST instantiations, sincos_fast off the
carry with the wave's exact fallback) must equal one sk_env_step launch per
tick bit for bit: state planes, every tick's done / winner, the RNG step
counter and the episode counters.  Random play with many restarts over both
state ports, both resident forms, both workgroup sizes and split launches
(the carry's keys miss at every launch start), and states and actions crafted
to force every fallback: move deltas at half-integers and next to them, fired
and in-flight projectiles whose step cannot be decided in fp32, rotations
outside the fast range, NaN / inf / -0.0 actions.  The crafted values are
checked on the CPU first (the kernels' formulas in numpy float32), so the
test cannot pass by never reaching the fallback.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PSPEED, QSPEED, LOOK = 3, 5, 0.25
FAST_RANGE = 1647099.3291652855


@pytest.fixture(scope="module")
def ssa():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import skillshot_learning_amd as m
    m.load_library()
    cfg = m._capi.default_config()
    assert (cfg.player_speed, cfg.projectile_speed, cfg.look_speed) == (PSPEED, QSPEED, LOOK)
    return m


def _env(monkeypatch, pol=1, pack=1, block="64"):
    monkeypatch.setenv("SK_MULTI_SPLIT", "1")
    monkeypatch.setenv("SK_MULTI_FAST", "1")
    monkeypatch.setenv("SK_MULTI_PACK", str(pack))
    monkeypatch.setenv("SK_MULTI_POLICY", str(pol))
    monkeypatch.setenv("SK_MULTI_BLOCK", block)


def _pair(ssa, n, seed, tick_limit):
    a = ssa.VecSkillshotGame(n, seed=seed, tick_limit=tick_limit)
    a.reset(random_positions=True)
    b = ssa.VecSkillshotGame(n, seed=seed, tick_limit=tick_limit)
    b.load_state_dict(a.state_dict())
    b.step_counter = a.step_counter
    return a, b


def _same_state(x, y):
    """Bitwise: a NaN rotation must match too."""
    sx, sy = x.state_dict(), y.state_dict()
    for k in sx:
        ax, ay = np.ascontiguousarray(sx[k]), np.ascontiguousarray(sy[k])
        assert ax.shape == ay.shape and ax.tobytes() == ay.tobytes(), k


def _stepwise(b, acts, T, R, slab0=0):
    wd, ww = [], []
    for t in range(T):
        o = b.step(acts[(slab0 + t) % R], obs=False, auto_reset=True)
        wd.append(o["done"].clone())
        ww.append(o["winner"].clone())
    return torch.stack(wd), torch.stack(ww)


def _check(a, b, acts, T, R, slab0=0):
    a.clear_counters()
    b.clear_counters()
    done, win = a.step_multi(acts, n_ticks=T, slab0=slab0, record=True)
    wd, ww = _stepwise(b, acts, T, R, slab0)
    torch.cuda.synchronize()
    assert torch.equal(done, wd)
    assert torch.equal(win, ww)
    _same_state(a, b)
    assert a.step_counter == b.step_counter
    ca, cb = a.counters(), b.counters()
    assert ca == cb
    return ca


# ------------------------------------------------------------- random play
@pytest.mark.parametrize("block", ["64", "512"], ids=["block64", "block512"])
@pytest.mark.parametrize("pack", [0, 1], ids=["form88", "packed"])
@pytest.mark.parametrize("pol", [0, 1], ids=["plain", "write_through"])
@pytest.mark.parametrize("n", [33, 3000])
def test_random_play_equals_stepwise(ssa, monkeypatch, pol, pack, block, n):
    """Tick limit 120 over 300 ticks: every game restarts several times; the
    last wave is partly filled."""
    _env(monkeypatch, pol, pack, block)
    T, R, slab0 = 300, 7, 3
    a, b = _pair(ssa, n, 21, 120)
    acts = a.gen_random_actions(R)
    c = _check(a, b, acts, T, R, slab0)
    assert c["dones"] > n


@pytest.mark.parametrize("pack", [0, 1], ids=["form88", "packed"])
@pytest.mark.parametrize("pol", [0, 1], ids=["plain", "write_through"])
def test_split_launches_equal_one(ssa, monkeypatch, pol, pack):
    """Launches of 1, 13 and 40 ticks against one of 54 and 54 single ticks:
    the carry's keys miss at every launch start, with projectiles in flight."""
    _env(monkeypatch, pol, pack)
    n, R = 3000, 11
    a, b = _pair(ssa, n, 4, 2000)
    c = ssa.VecSkillshotGame(n, seed=4, tick_limit=2000)
    c.load_state_dict(a.state_dict())
    c.step_counter = a.step_counter
    acts = a.gen_random_actions(R)
    for g in (a, b, c):
        g.clear_counters()
    s = 0
    for T in (1, 13, 40):
        d_last, w_last = a.step_multi(acts, n_ticks=T, slab0=s)
        s = (s + T) % R
    d_all, w_all = b.step_multi(acts, n_ticks=54, slab0=0, record=True)
    wd, ww = _stepwise(c, acts, 54, R)
    torch.cuda.synchronize()
    assert torch.equal(d_all, wd) and torch.equal(w_all, ww)
    assert torch.equal(d_last, wd[-1]) and torch.equal(w_last, ww[-1])
    _same_state(a, c)
    _same_state(b, c)
    assert a.step_counter == b.step_counter == c.step_counter
    assert a.counters() == b.counters() == c.counters()


# ----------------------------------------- the kernels' formulas in float32
# (csrc/sk_trig.hpp).  fmaf is taken as the float32 rounding of the float64
# a * b + c: the product is exact there, and the second rounding can move the
# result by one float32 ulp at most, 6e-8 on these values, against margins of
# 1e-6 and more in every assertion below.
F = np.float32


def _fma(a, b, c):
    return F(np.float64(a) * np.float64(b) + np.float64(c))


def _poly(yf):
    z = F(yf * yf)
    ps = _fma(_fma(F(-1.9515295891e-4), z, F(8.3321608736e-3)), z, F(-1.6666654611e-1))
    pc = _fma(_fma(F(2.443315711809948e-5), z, F(-1.388731625493765e-3)), z, F(4.166664568298827e-2))
    return _fma(F(yf * z), ps, yf), _fma(F(z * z), pc, _fma(F(-0.5), z, F(1.0)))


def sincos_fast(x):
    x = np.float64(x)
    ok = bool(abs(x) < FAST_RANGE)
    if not ok:
        return F(0), F(1), False
    fn = np.rint(x * 6.36619772367581382433e-01)
    y = (x - fn * 1.57079632673412561417e+00) - fn * 6.07710050630396597660e-11
    ks, kc = _poly(F(y))
    n = int(fn) & 3
    s, c = (kc, ks) if n & 1 else (ks, kc)
    if n in (1, 2):
        c = F(-c)
    if n >= 2:
        s = F(-s)
    return s, c, True


def sincos_add(s, c, d):
    ks, kc = _poly(F(d))
    return _fma(s, kc, F(c * ks)), _fma(c, kc, F(-F(s * ks)))


def round_safe(d, eps):
    d = F(d)  # NaN / inf: not safe
    if not np.isfinite(d):
        return False
    t = F(d - np.floor(d))
    return bool(abs(F(t - F(0.5))) > F(eps))


def clampf(a):
    a = F(a)
    a = F(1.0) if a >= 1.0 else a
    a = F(-1.0) if a <= -1.0 else a
    return a


def move_safe(rot, a):
    s, c, ok = sincos_fast(rot)
    sp, al = F(PSPEED), clampf(a)
    eps = F(1e-6) * sp
    return ok and round_safe(F(F(s * sp) * al), eps) and round_safe(F(F(c * sp) * al), eps)


def fired_safe(rot, look):
    s, c, ok = sincos_fast(rot)
    us, uc = sincos_add(s, c, F(clampf(look) * F(LOOK)))
    sp = F(QSPEED)
    eps = F(2e-6) * sp
    return ok and round_safe(F(us * sp), eps) and round_safe(F(uc * sp), eps)


def flight_safe(qrot):
    s, c, ok = sincos_fast(qrot)
    sp = F(QSPEED)
    eps = F(2e-6) * sp
    return ok and round_safe(F(s * sp), eps) and round_safe(F(c * sp), eps)


# ------------------------------------------------------- forced fallbacks
N_CRAFT = 130  # 260 lanes: four full waves and a last one of four lanes


def _slots(k):
    """k distinct (game, player) places: the ragged last wave's games first,
    the others spread over the full waves among ordinary lanes."""
    s = [(128, 0), (129, 1)] + [((3 * i + 1) % 128, i % 2) for i in range(128)]
    assert k <= len(s)
    return s[:k]


def _crafted(ssa, seed, tick_limit, edit):
    """Two equal envs from a random start with `edit(state)` applied."""
    a, b = _pair(ssa, N_CRAFT, seed, tick_limit)
    st = a.state_dict()
    edit(st)
    for g in (a, b):
        g.load_state_dict(st)
    return a, b


def _place(st, g, p, rot, cooldown, pos=(125, 125)):
    st["rot"][g, p] = rot
    st["pos"][g, 2 * p:2 * p + 2] = pos
    st["qcdage"][g, 2 * p] = cooldown


def _tie_rotations(speed):
    """Rotations whose sine (asin) or cosine (acos) times `speed` is a
    half-integer: (rotation, must_fail) with the neighbours that stay inside
    the bound, and the probes 1e-6 away, which may fall either side of it."""
    out = []
    for k in range(1, 2 * speed, 2):
        for r0 in (math.asin(k / (2.0 * speed)), math.acos(k / (2.0 * speed))):
            for r in (r0, np.nextafter(r0, 10.0), np.nextafter(r0, -10.0), r0 + 1e-9, r0 - 1e-9):
                out.append((float(r), True))
            out += [(r0 + 1e-6, False), (r0 - 1e-6, False)]
    return out


@pytest.mark.parametrize("pack", [0, 1], ids=["form88", "packed"])
@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["forwards", "backwards"])
def test_move_ties(ssa, monkeypatch, pack, sign):
    """|d| = 0.5, 1.5, 2.5 at move action +-1 with no look: the rotation
    stays, so the lane's move is undecidable in fp32 on every tick."""
    rots = _tie_rotations(PSPEED)
    for r, must in rots:
        assert not must or not move_safe(r, sign), r
    assert sum(not move_safe(r, sign) for r, _ in rots) >= 30
    slots = _slots(len(rots))

    def edit(st):
        for (g, p), (r, _) in zip(slots, rots):
            _place(st, g, p, r, 1000)

    _env(monkeypatch, 1, pack)
    T, R = 40, 5
    a, b = _crafted(ssa, 11, 2000, edit)
    acts = a.gen_random_actions(R)
    for (g, p) in slots:
        acts[:, p, g, 0] = sign
        acts[:, p, g, 1] = 0.0
    _check(a, b, acts, T, R)


@pytest.mark.parametrize("pack", [0, 1], ids=["form88", "packed"])
def test_fired_projectile_ties(ssa, monkeypatch, pack):
    """Cooldown 0 and rot = r0 - l * look with sin or cos of r0 times the
    projectile speed a half-integer: the step of the projectile fired on the
    first tick is exact-only for its whole flight (60 ticks: to the wall)."""
    look = 0.5
    rots = [(r - look * LOOK, must) for r, must in _tie_rotations(QSPEED)]
    for r, must in rots:
        assert not must or not fired_safe(r, look), r
    slots = _slots(len(rots))

    def edit(st):
        for (g, p), (r, _) in zip(slots, rots):
            _place(st, g, p, r, 0)

    _env(monkeypatch, 1, pack)
    T, R = 60, 64
    a, b = _crafted(ssa, 12, 2000, edit)
    acts = a.gen_random_actions(R)
    for (g, p) in slots:
        acts[0, p, g, 1] = look
    _check(a, b, acts, T, R)


@pytest.mark.parametrize("pack", [0, 1], ids=["form88", "packed"])
def test_in_flight_ties_at_launch_start(ssa, monkeypatch, pack):
    """A projectile already in flight with such a rotation when the launch
    starts: the key misses and sincos_fast of its rotation cannot decide."""
    rots = _tie_rotations(QSPEED)
    for r, must in rots:
        assert not must or not flight_safe(r), r
    slots = _slots(len(rots))

    def edit(st):
        for (g, p), (r, _) in zip(slots, rots):
            _place(st, g, p, 0.3 * g, 70)
            st["qrot"][g, p] = r
            st["qpos"][g, 2 * p:2 * p + 2] = (120, 130)
            st["qcdage"][g, 2 * p + 1] = 3
            fl = int(st["misc"][g, 1]) & 0xFFFFFFFF
            st["misc"][g, 1] = np.int32((fl | (1 << (8 * p)) | (1 << 16)) & 0x7FFFFFFF)

    _env(monkeypatch, 1, pack)
    T, R = 60, 9
    a, b = _crafted(ssa, 13, 2000, edit)
    acts = a.gen_random_actions(R)
    _check(a, b, acts, T, R)


@pytest.mark.parametrize("pack", [0, 1], ids=["form88", "packed"])
def test_rotations_outside_the_fast_range(ssa, monkeypatch, pack):
    below, above = float(np.nextafter(FAST_RANGE, 0.0)), FAST_RANGE
    rots = [below, -below, above, -above, np.nextafter(above, 1e9), 1647100.0, -1647100.0, 2.0 ** 40, -2.0 ** 40,
            2.0 ** 40 + 0.25, 1e15]
    assert sincos_fast(below)[2] and sincos_fast(-below)[2]
    for r in rots[2:]:
        assert not sincos_fast(r)[2], r
    slots = _slots(2 * len(rots))

    def edit(st):
        for i, (g, p) in enumerate(slots):
            _place(st, g, p, rots[i % len(rots)], 0 if i < len(rots) else 25)

    _env(monkeypatch, 1, pack)
    T, R = 60, 7
    a, b = _crafted(ssa, 14, 2000, edit)
    acts = a.gen_random_actions(R)
    _check(a, b, acts, T, R)


@pytest.mark.parametrize("pack", [0, 1], ids=["form88", "packed"])
def test_special_actions(ssa, monkeypatch, pack):
    """NaN and +-inf move and look actions (a NaN move never commits, a NaN
    look makes the rotation NaN from then on), and -0.0 at rotation +-0.0."""
    nan, inf = float("nan"), float("inf")
    cases = [(0.7, nan, 0.2), (0.7, 0.4, nan), (0.7, nan, nan), (1.9, inf, -inf), (1.9, -inf, inf),
             (0.0, -0.0, 0.0), (-0.0, -0.0, -0.0), (-0.0, 1.0, 0.0), (0.0, -1.0, -0.0)]
    for r, am, al in cases[:3]:
        assert not (move_safe(r, am) and fired_safe(r, al))
    slots = _slots(2 * len(cases))

    def edit(st):
        for i, (g, p) in enumerate(slots):
            _place(st, g, p, cases[i % len(cases)][0], 0 if i < len(cases) else 25)

    _env(monkeypatch, 1, pack)
    T, R = 30, 4
    a, b = _crafted(ssa, 15, 2000, edit)
    acts = a.gen_random_actions(R)
    for i, (g, p) in enumerate(slots):
        _, am, al = cases[i % len(cases)]
        acts[0, p, g, 0] = am
        acts[0, p, g, 1] = al
        if i % 2:  # ... and on every tick
            acts[:, p, g, 0] = am
            acts[:, p, g, 1] = al
    _check(a, b, acts, T, R)


# --------------------------------------------------------------- the others
def test_default_selection_at_40960_games(ssa, monkeypatch):
    """No switch set: 40,960 games in a launch of 100 ticks run the fast form
    by default (the packed split kernel's smallest size, the shortest launch
    that selects it), a launch of 20 ticks the fp64 carry; both equal the
    single ticks."""
    for k in ("SK_MULTI_SPLIT", "SK_MULTI_FAST", "SK_MULTI_PACK", "SK_MULTI_POLICY", "SK_MULTI_BLOCK"):
        monkeypatch.delenv(k, raising=False)
    n, R = 40960, 6
    a, b = _pair(ssa, n, 3, 60)
    acts = a.gen_random_actions(R)
    _check(a, b, acts, 100, R, 1)
    _check(a, b, acts, 20, R, 5)


def test_cpu_backend_equals_gpu(ssa, monkeypatch):
    _env(monkeypatch, 1, 1)
    n, T, R = 3000, 260, 5
    g = ssa.VecSkillshotGame(n, seed=9, tick_limit=100)
    g.reset(random_positions=True)
    c = ssa.VecSkillshotGame(n, device="cpu", seed=9, tick_limit=100)
    c.load_state_dict(g.state_dict())
    acts = g.gen_random_actions(R)
    g.clear_counters()
    c.clear_counters()
    dg, wg = g.step_multi(acts, n_ticks=T, slab0=2, record=True)
    dc, wc = c.step_multi(acts.cpu(), n_ticks=T, slab0=2, record=True)
    assert np.array_equal(dg.cpu().numpy(), dc.numpy())
    assert np.array_equal(wg.cpu().numpy(), wc.numpy())
    _same_state(g, c)
    assert g.counters() == c.counters()


def test_graph_captured_launch(ssa, monkeypatch):
    _env(monkeypatch, 1, 0)
    n, T, R = 3000, 30, 4
    a, b = _pair(ssa, n, 5, 25)
    acts = a.gen_random_actions(R)
    done = torch.zeros(n, dtype=torch.uint8, device="cuda")
    a.clear_counters()
    b.clear_counters()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        a.step_multi_raw(ctypes.c_void_p(acts.data_ptr()), R, 0, T, ctypes.c_void_p(done.data_ptr()), None, 0,
                         stream=ctypes.c_void_p(st.cuda_stream))
    with torch.cuda.stream(st):
        g.replay()
    st.synchronize()
    wd, _ = _stepwise(b, acts, T, R)
    torch.cuda.synchronize()
    assert torch.equal(done, wd[-1])
    _same_state(a, b)
    assert a.step_counter == b.step_counter
    assert a.counters() == b.counters()
