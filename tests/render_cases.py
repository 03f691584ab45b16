"""States and expected boards shared by test_render_cpu.py and
test_render_gpu.py: the reference's own boards (tests/golden/boards.npz) and
an edge set whose expected board is the reference painter
(game.rasterize_board, SkillshotGame.py:36-56) on a canvas padded by PAD
cells per side and cropped: the painter, clipped."""
import math

import numpy as np

import golden_replay as gr
from skillshot_learning_amd.game import rasterize_board

PAD = 8


def padded_painter(W, H, pos, rot, qpos, qvalid):
    """uint8 [W, H]: rasterize_board of one state on a (W + 2 PAD, H + 2 PAD)
    canvas, cropped.  A projectile that is not drawn may be anywhere."""
    shift = lambda xy: [int(xy[0]) + PAD, int(xy[1]) + PAD]
    q = [shift(qpos[k]) if qvalid[k] else [0, 0] for k in range(2)]
    canvas = rasterize_board(np.zeros((W + 2 * PAD, H + 2 * PAD), dtype=np.int64), [shift(pos[0]), shift(pos[1])],
                             [float(rot[0]), float(rot[1])], q, [int(qvalid[0]), int(qvalid[1])])
    return canvas[PAD:PAD + W, PAD:PAD + H].astype(np.uint8)


def planes_of(pos, rot, qpos, qvalid):
    """load_state_dict planes of live games from [K, 2, 2] positions, [K, 2]
    rotations and [K, 2] projectile-valid flags"""
    pos, qpos = np.asarray(pos, np.int64), np.asarray(qpos, np.int64)
    k = pos.shape[0]
    qv = np.asarray(qvalid, np.int64)
    flags = (qv[:, 0] | (qv[:, 1] << 8) | (1 << 16)).astype(np.int32)
    return dict(pos=pos.reshape(k, 4).astype(np.int32), rot=np.asarray(rot, np.float64).reshape(k, 2),
                qpos=qpos.reshape(k, 4).astype(np.int32), qrot=np.zeros((k, 2)),
                qcdage=np.zeros((k, 4), np.int32), misc=np.stack([np.zeros(k, np.int32), flags], -1))


def edge_states(W, H):
    """the edge set on a W x H board: (pos [K,2,2], rot [K,2], qpos [K,2,2], qvalid [K,2])"""
    S = []

    def add(p1, p2, r=(0.0, 0.0), q1=(0, 0), q2=(0, 0), v=(0, 0)):
        S.append(([list(p1), list(p2)], list(r), [list(q1), list(q2)], list(v)))

    mid1, mid2 = (W // 4, H // 4), (W // 2 + 3, H // 2 + 2)
    # players in the corners, a projectile in the far corner; and swapped
    add((0, 0), (W - 5, H - 5), q1=(W - 3, H - 3), v=(1, 0))
    add((W - 5, H - 5), (0, 0), q2=(W - 3, H - 3), q1=(0, 0), v=(1, 1))
    add((0, H - 5), (W - 5, 0), r=(1.0, -2.0))
    # a valid projectile straddling each edge, and the corners
    add(mid1, mid2, q1=(-1, 7), q2=(W - 1, 9), v=(1, 1))
    add(mid1, mid2, q1=(7, -1), q2=(9, H - 1), v=(1, 1))
    add(mid1, mid2, q1=(-2, H - 2), q2=(W - 2, -2), v=(1, 1))
    add(mid1, mid2, q1=(-1, -1), q2=(W - 1, H - 1), v=(1, 1))
    add(mid1, mid2, q1=(-3, 5), q2=(5, H), v=(1, 1))  # just off the board: nothing drawn
    # players partly off the board (loaded states only): clipped
    add((-2, H - 3), (W - 2, -4), r=(math.pi / 2, 0.5))
    add((-5, 3), (3, H), r=(0.3, 0.4))  # wholly off
    # painter's order: p1's projectile over p2's body, p2's over p1's, both, and over the pointers
    add(mid1, mid2, q1=(mid2[0] + 1, mid2[1] + 1), v=(1, 0))
    add(mid1, mid2, q2=(mid1[0] + 1, mid1[1] + 1), v=(0, 1))
    add(mid1, mid2, q1=mid2, q2=mid1, v=(1, 1))
    add(mid1, mid2, r=(0.0, math.pi / 2), q1=(mid2[0] - 1, mid2[1] + 1), q2=(mid1[0] + 1, mid1[1] - 2), v=(1, 1))
    add(mid1, mid2, q1=mid1, q2=mid1, v=(1, 1))  # both projectiles on one cell: p2's wins
    # both players on the same cell, and overlapping by one column
    add(mid1, mid1, r=(0.0, math.pi))
    add(mid1, (mid1[0] + 4, mid1[1] + 1), r=(-math.pi / 2 + 0.1, math.pi / 2 - 0.1))
    # rotations: the pointer on a border cell of the 5x5, and not drawn at index 5
    rots = [0.0, -0.0, math.pi / 2, -math.pi / 2, math.pi, 1e8, -1e8, -math.pi, 3 * math.pi / 2, 0.7, -2.4]
    for i, r in enumerate(rots):
        add(mid1, mid2, r=(r, rots[(i + 3) % len(rots)]))
    # each qvalid combination; an invalid projectile far away is never drawn
    for v in ((0, 0), (1, 0), (0, 1), (1, 1)):
        add(mid1, mid2, q1=(3, H - 4), q2=(W - 4, 2), v=v)
    add(mid1, mid2, q1=(-900, 10 ** 6), q2=(10 ** 6, -900), v=(0, 0))
    add(mid1, mid2, q1=(-900, 10 ** 6), q2=(5, 5), v=(0, 1))
    pos, rot, qpos, qv = (np.array([s[i] for s in S]) for i in range(4))
    return pos, rot.astype(np.float64), qpos, qv


def expected_boards(W, H, pos, rot, qpos, qvalid):
    return np.stack([padded_painter(W, H, pos[k], rot[k], qpos[k], qvalid[k]) for k in range(len(pos))])


def golden_states():
    """(planes, boards): every state of tests/golden/boards.npz and the reference's board of it"""
    d = gr.load("boards")
    return planes_of(d["pos"], d["rot"], d["qpos"], d["qvalid"]), d["board"].astype(np.uint8)


def default_cases():
    """(planes, boards) of the fixtures followed by the edge set at the reference's 250 x 250"""
    gp, gb = golden_states()
    e = edge_states(250, 250)
    ep, eb = planes_of(*e), expected_boards(250, 250, *e)
    return {k: np.concatenate([gp[k], ep[k]]) for k in gp}, np.concatenate([gb, eb])


SMALL = (41, 23)  # 943 cells: odd, so board bases fall on every residue mod 16


def small_config(ssa_capi):
    c = ssa_capi.default_config()
    c.board_w, c.board_h = SMALL
    c.fixed_p1_x, c.fixed_p1_y, c.fixed_p2_x, c.fixed_p2_y = 5, 5, 30, 15
    c.rand_lo, c.rand_hi = 0, 18
    return c


def small_cases():
    """five states on the 41 x 23 board with sprites at both ends of their
    boards (the chunks that straddle two boards carry cells of both)"""
    W, H = SMALL
    pos, rot, qpos, qv = edge_states(W, H)
    pick = [0, 1, 2, 6, 12]
    e = (pos[pick], rot[pick], qpos[pick], qv[pick])
    return planes_of(*e), expected_boards(W, H, *e)
