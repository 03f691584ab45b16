"""The four scripted policies restated in plain Python (a helper, not a test):
math.sin / math.cos on state arrays in the engine's plane layout, the C
oracle's keyed draw for `random`.  Independent of csrc/sk_bot.hpp: the tests
compare the engine's sk_env_bot_act and the actions the match paths record
against this.

Tolerances (tests use them as they stand): `still` is zero and `random` the
oracle's floats, both exact; `move` of aimer / chaser is 0 or 1 from an
integer compare, exact; `look` is continuous in the state except on the tie
side == 0 with ahead <= 0, libm and the engine's sincos differ by ulps of fp64
and the result is O(1) in fp32 (half an ulp: 6e-8), so 1e-6 absolute.
"""
import math

import numpy as np

from oracle import oracle

KINDS = ("still", "random", "aimer", "chaser")
LOOK_TOL = 1e-6


def look_of(rot, dx, dy, look_speed):
    s, c = math.sin(rot), math.cos(rot)
    side = s * dy - c * dx
    ahead = -(s * dx) - c * dy
    if ahead > 0:
        t = side / (ahead * look_speed)
        return 1.0 if t >= 1 else -1.0 if t <= -1 else t
    return -1.0 if side < 0 else 1.0


def actions(kind, pos, rot, look_speed=0.1, player_size=5, seed=0, env_offset=0, step=0):
    """float32 [2, N, 2] of `kind` on pos int [N, 4] (x1, y1, x2, y2) and rot
    float64 [N, 2]; seed / env_offset / step: the random policy's key"""
    pos, rot = np.asarray(pos).astype(np.int64).reshape(-1, 4), np.asarray(rot, np.float64).reshape(-1, 2)
    n = pos.shape[0]
    out = np.zeros((2, n, 2), np.float32)
    if kind == "still":
        return out
    if kind == "random":
        st = oracle.OracleState(n, seed=seed, env_offset=env_offset)
        st.step_counter = int(step)
        return st.gen_random_actions(1)[0]
    assert kind in ("aimer", "chaser"), kind
    near = 8 * int(player_size)
    for i in range(n):
        for p in range(2):
            o = 1 - p
            dx, dy = int(pos[i, 2 * o] - pos[i, 2 * p]), int(pos[i, 2 * o + 1] - pos[i, 2 * p + 1])
            out[p, i, 1] = np.float32(look_of(float(rot[i, p]), dx, dy, float(look_speed)))
            if kind == "chaser":
                out[p, i, 0] = 1.0 if dx * dx + dy * dy > near * near else 0.0
    return out


def assert_actions(kind, got, want, where=""):
    """`got` against this file's `want` under the tolerances above"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (where, got.shape, want.shape)
    if kind in ("still", "random"):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{where}: {kind} differs"
        return
    assert np.array_equal(got[..., 0], want[..., 0]), f"{where}: {kind} move differs"
    err = np.abs(got[..., 1].astype(np.float64) - want[..., 1].astype(np.float64)).max() if got.size else 0.0
    assert err <= LOOK_TOL, f"{where}: {kind} look off by {err}"
