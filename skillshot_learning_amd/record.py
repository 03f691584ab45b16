"""MatchRecord — what the games of a head-to-head match did at every tick.

`evaluate`, `league` and the env's `act_match` / `act_league` play whole
matches and return tallies; with `record=` they also keep, for the first games
of every block of games (a match is one block, a league's blocks are its
pairings), each tick's state, both seats' actions and rewards, and the final
state.  On a GPU the one-launch match kernels write the record themselves
(sk_env_act_match_rec / sk_env_act_league_rec); the per-tick loop
path (CPU backend, bf16 or torch actors, SK_MATCH_KERNEL=0) fills the same
object, so a record does not depend on the path that made it.

Layout: S slabs of R rows.  Row j is one recorded game, slab s its state
after s ticks of the match: states[plane][s, j] in the engine's plane layout
(vec_env.PLANES), actions[s, p, j] = the (speed, look) seat p + 1 acted with
on state s, rewards[s, p, j] = that seat's reward for the tick.  Row j holds
slabs 0 .. lengths[j] and lengths[j] actions and rewards; what lies past them
was never written (zero in a record allocated here).
"""
import ctypes

import numpy as np
import torch

from . import _capi
from ._capi import check

_PLANES = (("pos", torch.int32, 4), ("rot", torch.float64, 2), ("qpos", torch.int32, 4),
           ("qrot", torch.float64, 2), ("qcdage", torch.int32, 4), ("misc", torch.int32, 2))  # vec_env.PLANES


def _copy_config(cfg):
    c = _capi.SkConfig()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(cfg), ctypes.sizeof(c))
    return c


class MatchRecord:
    """states   {plane: [S, R, width]}
    actions  float32 [S - 1, 2, R, 2]
    rewards  float32 [S - 1, 2, R]
    lengths  int32 [R]: the ticks each row's game played in the match
    games    int64 [R]: each row's game index (in the env that played it;
             SkillshotLearner.league: among the pairing's games)
    pairs    None, or for a league one (seat-1 actor, seat-2 actor) per row
    config   the sk_config the games were played with
    per_block  the rows each block of games contributes (R = blocks * per_block)
    ticks_run  the ticks the calls that filled the record ran: where a resumed
             call continues (its slab0)"""

    def __init__(self, states, actions, rewards, lengths, games, config, pairs=None, per_block=None, ticks_run=0):
        self.states = {name: states[name] for name, _, _ in _PLANES}
        self.actions, self.rewards, self.lengths, self.games = actions, rewards, lengths, games
        self.config = _copy_config(config)
        self.pairs = None if pairs is None else [(int(i), int(j)) for i, j in pairs]
        self.per_block = int(self.rows if per_block is None else per_block)
        self.ticks_run = int(ticks_run)

    @classmethod
    def allocate(cls, slabs, games, config, device, per_block=None, pairs=None):
        """an empty (all-zero) record of `slabs` slabs for the games `games`
        (their indices, one per row) on `device`"""
        S, dev = int(slabs), torch.device(device)
        games = torch.as_tensor(games, dtype=torch.int64).reshape(-1).to(dev)
        R = games.numel()
        if S < 2 or R < 1:
            raise ValueError("a record needs at least 2 slabs and 1 row")
        states = {name: torch.zeros((S, R, w), dtype=dt, device=dev) for name, dt, w in _PLANES}
        return cls(states, torch.zeros((S - 1, 2, R, 2), dtype=torch.float32, device=dev),
                   torch.zeros((S - 1, 2, R), dtype=torch.float32, device=dev),
                   torch.zeros(R, dtype=torch.int32, device=dev), games, config, pairs=pairs, per_block=per_block)

    # ------------------------------------------------------------------ shape
    @property
    def slabs(self):
        return self.states["misc"].shape[0]

    @property
    def rows(self):
        return self.states["misc"].shape[1]

    @property
    def device(self):
        return self.states["misc"].device

    def __len__(self):
        return self.rows

    def check_layout(self, rows, device):
        """raise unless this record can take a launch's stores: `rows` rows on
        `device`, every tensor contiguous and of its dtype and shape"""
        S, R = self.slabs, self.rows
        want = [(self.states[name], (S, R, w), dt) for name, dt, w in _PLANES]
        want += [(self.actions, (S - 1, 2, R, 2), torch.float32), (self.rewards, (S - 1, 2, R), torch.float32),
                 (self.lengths, (R,), torch.int32), (self.games, (R,), torch.int64)]
        for t, shape, dt in want:
            if tuple(t.shape) != shape or t.dtype != dt or t.device != device or not t.is_contiguous():
                raise ValueError(f"record tensors must be contiguous on {device}: {dt} {shape} expected, "
                                 f"{t.dtype} {tuple(t.shape)} on {t.device} found")
        if R != rows:
            raise ValueError(f"the record has {R} rows, the call records {rows}")

    def c_struct(self, slab0):
        """the sk_match_record of a launch that continues at slab `slab0`"""
        view = _capi.SkStateView(self.slabs * self.rows, *[self.states[name].data_ptr() for name, _, _ in _PLANES])
        return _capi.SkMatchRecord(view, self.actions.data_ptr(), self.rewards.data_ptr(), self.slabs, self.rows,
                                   self.per_block, int(slab0))

    # ------------------------------------------------------------------ reading
    def _length(self, j):
        j = int(j)
        if not 0 <= j < self.rows:
            raise IndexError(f"row {j} outside [0, {self.rows})")
        return j, min(int(self.lengths[j]), self.slabs - 1)

    def game(self, j):
        """row j's game: dict(states {plane: [L + 1, width]}, actions [L, 2, 2]
        (tick, player, {speed, look}: trace_game's layout), rewards [L, 2],
        length L)"""
        j, L = self._length(j)
        return dict(states={name: t[:L + 1, j] for name, t in self.states.items()},
                    actions=self.actions[:L, :, j], rewards=self.rewards[:L, :, j], length=L)

    def boards(self, j):
        """the boards of row j's states (SkillshotGame.get_board of each):
        uint8 [L + 1, W, H] on the record's device, one sk_render_states
        launch over the row's valid slabs"""
        j, L = self._length(j)
        dev = self.device
        planes = [self.states[name][:L + 1, j].contiguous() for name, _, _ in _PLANES]
        out = torch.empty((L + 1, self.config.board_w, self.config.board_h), dtype=torch.uint8, device=dev)
        view = _capi.SkStateView(L + 1, *[t.data_ptr() for t in planes])
        cpu = dev.type == "cpu"
        stream = None if cpu else ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        check(_capi.load().sk_render_states(ctypes.byref(self.config), -1 if cpu else dev.index, ctypes.byref(view),
                                            None, L + 1, ctypes.c_void_p(out.data_ptr()), stream))
        return out

    def board_sequences(self, include_start=False):
        """one int8 numpy array [L, W, H] per row, the boards after each tick
        (with include_start [L + 1, W, H], the start first): what
        save_training_boards takes, so the reference's replay viewer plays a
        recorded match as it plays a training run"""
        return [self.boards(j)[0 if include_start else 1:].to(torch.int8).cpu().numpy() for j in range(self.rows)]

    def cpu(self):
        """this record with every tensor on the host (itself if it is there)"""
        return self.to("cpu")

    def to(self, device):
        dev = torch.device(device)
        if dev == self.device:
            return self
        return MatchRecord({name: t.to(dev) for name, t in self.states.items()}, self.actions.to(dev),
                           self.rewards.to(dev), self.lengths.to(dev), self.games.to(dev), self.config,
                           pairs=self.pairs, per_block=self.per_block, ticks_run=self.ticks_run)

    @staticmethod
    def concat(records, pairs=None):
        """records of the same slabs side by side, rows in the order given
        (SkillshotLearner.league's pair-by-pair path); pairs: one (i, j) per
        record, repeated for its rows"""
        first = records[0]
        rows_pairs = None if pairs is None else [pr for r, pr in zip(records, pairs) for _ in range(r.rows)]
        return MatchRecord({name: torch.cat([r.states[name] for r in records], 1) for name, _, _ in _PLANES},
                           torch.cat([r.actions for r in records], 2), torch.cat([r.rewards for r in records], 2),
                           torch.cat([r.lengths for r in records]), torch.cat([r.games for r in records]),
                           first.config, pairs=rows_pairs, per_block=first.per_block, ticks_run=first.ticks_run)

    # ------------------------------------------------------------------ the per-tick loop's side
    def loop_before(self, g, t, alive):
        """the loop path, before tick t: the pre-tick state of the rows whose
        game is alive (`alive`: bool [N] over env g's games)"""
        ar = alive[self.games]
        if t < self.slabs - 1:
            for name, _, _ in _PLANES:
                dst = self.states[name][t]
                dst.copy_(torch.where(ar[:, None], getattr(g, name)[self.games], dst))
        return ar

    def loop_after(self, g, t, ar, act, reward, done):
        """the loop path, after tick t: the tick's actions [2, N, 2] and
        rewards [2, N] of the rows that played it and the post-tick state of
        those that ended on it (the loop keeps moving ended games: their later
        states are not the game's)"""
        if t >= self.slabs - 1:
            return
        rg = self.games
        self.actions[t].copy_(torch.where(ar[None, :, None], act[:, rg], self.actions[t]))
        self.rewards[t].copy_(torch.where(ar[None, :], reward[:, rg], self.rewards[t]))
        ended = ar & done[rg].bool()
        for name, _, _ in _PLANES:
            dst = self.states[name][t + 1]
            dst.copy_(torch.where(ended[:, None], getattr(g, name)[rg], dst))


def config_arrays(cfg):
    """an sk_config as named numpy scalars (persist.save_match_record)"""
    return {f"config_{name}": np.asarray(getattr(cfg, name)) for name, _ in _capi.SkConfig._fields_}


def config_from_arrays(d):
    cfg = _capi.SkConfig()
    for name, ctype in _capi.SkConfig._fields_:
        v = d[f"config_{name}"]
        setattr(cfg, name, float(v) if ctype is ctypes.c_double else int(v))
    return cfg
