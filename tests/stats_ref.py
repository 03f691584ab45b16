"""The match statistics restated in plain Python (a helper, not a test):
numpy / math over a full MatchRecord (record=games), the pre-tick states of
slabs 0 .. lengths - 1 of every row.  Independent of csrc/sk_stats.hpp: the
tests compare the engine's tallies against this.

Every statistic is an integer.  All but `on_target` come from integer compares
and are exact.  `on_target` compares fp64 products of math.sin / math.cos,
which need not be the engine's sincos to the last bit: a (row, tick, seat)
whose |fabs(side) - player_size| or |ahead| is within EDGE of the decision is
reported as undecided, and the tests compare `on_target` only for (row, seat)
without an undecided tick.
"""
import math

import numpy as np

NAMES = ("shots", "in_flight", "on_target", "under_fire", "at_wall", "path", "dist_sum", "closest")
FAR = 2 ** 31 - 1
EDGE = 1e-9


def of_record(rec):
    """(stats int64 [8, 2, R], undecided bool [2, R]: on_target has a tick too
    close to call, cases: the (row, tick, seat) cases seen, close: how many of
    them were too close to call)"""
    rec = rec.cpu()
    cfg = rec.config
    size, speed, W, H = int(cfg.player_size), int(cfg.player_speed), int(cfg.board_w), int(cfg.board_h)
    R = rec.rows
    out = np.zeros((8, 2, R), np.int64)
    out[7] = FAR
    undecided = np.zeros((2, R), bool)
    cases = close = 0
    pos, rot = rec.states["pos"].numpy().astype(np.int64), rec.states["rot"].numpy()
    qpos, ca = rec.states["qpos"].numpy().astype(np.int64), rec.states["qcdage"].numpy().astype(np.int64)
    flags = rec.states["misc"].numpy()[..., 1].astype(np.int64) & 0xFFFFFFFF
    for j in range(R):
        prev = [None, None]
        for t in range(int(rec.lengths[j])):
            for p in range(2):
                o = 1 - p
                x, y = int(pos[t, j, 2 * p]), int(pos[t, j, 2 * p + 1])
                ox, oy = int(pos[t, j, 2 * o]), int(pos[t, j, 2 * o + 1])
                dx, dy = ox - x, oy - y
                cheb = max(abs(dx), abs(dy))
                s, c = math.sin(float(rot[t, j, p])), math.cos(float(rot[t, j, p]))
                side = s * dy - c * dx
                ahead = -(s * dx) - c * dy
                cases += 1
                if abs(abs(side) - size) <= EDGE or abs(ahead) <= EDGE:
                    undecided[p, j] = True
                    close += 1
                own = (int(flags[t, j]) >> (8 * p)) & 0xFF
                opp = (int(flags[t, j]) >> (8 * o)) & 0xFF
                fx, fy = int(qpos[t, j, 2 * o]), int(qpos[t, j, 2 * o + 1])
                out[0, p, j] += int(ca[t, j, 2 * p]) <= 0
                out[1, p, j] += own != 0
                out[2, p, j] += ahead > 0 and abs(side) <= size
                out[3, p, j] += opp != 0 and max(abs(fx - x), abs(fy - y)) <= 2 * size
                out[4, p, j] += x < speed or y < speed or x + size + speed > W or y + size + speed > H
                if prev[p] is not None:
                    out[5, p, j] += abs(x - prev[p][0]) + abs(y - prev[p][1])
                prev[p] = (x, y)
                out[6, p, j] += cheb
                out[7, p, j] = min(int(out[7, p, j]), cheb)
    return out, undecided, cases, close
