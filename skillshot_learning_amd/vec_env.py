"""VecSkillshotGame — N Skillshot games stepped on one MI355X by libskillshot.

State lives in HBM as torch tensors (the struct-of-arrays layout of
include/skillshot.h) that the C engine is attached to, so observations,
rewards and the state itself are torch tensors with no copies.  Every method
is the batched form of a reference method (cited per method); the fused
`step` is the learner's whole per-tick protocol (SkillshotLearner.py:302-324)
in one kernel launch.
"""
import ctypes

import numpy as np
import torch

from . import _capi
from ._capi import SkillshotError, check
from .scripted import ScriptedActor, kind_code

PLANES = (("pos", torch.int32, 4), ("rot", torch.float64, 2), ("qpos", torch.int32, 4),
          ("qrot", torch.float64, 2), ("qcdage", torch.int32, 4), ("misc", torch.int32, 2))

REWARD_KINDS = {"looking": _capi.SK_REWARD_LOOKING, "simple": _capi.SK_REWARD_SIMPLE}

# get_state per-player key order (SkillshotGame.py:145-163); sk_env_features columns
FEATURE_KEYS = ("player_grad", "player_x_dir", "player_path_dist_opponent", "player_dist_opponent",
                "player_pos_x", "player_pos_y", "player_rotation", "projectile_cooldown",
                "projectile_grad", "projectile_x_dir", "projectile_path_dist_opponent",
                "projectile_pos_x", "projectile_pos_y", "projectile_rotation", "projectile_age",
                "projectile_valid", "projectile_dist_opponent", "projectile_future_collision_opponent")


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _resolve_device(device):
    """cuda[:i] -> the gfx950 engine on that device; cpu -> libskillshot's CPU
    backend (device = -1, csrc/sk_host.cpp), chosen explicitly, never as a
    fallback: a cuda request without a GPU raises."""
    dev = torch.device(device)
    if dev.type == "cpu":
        return dev
    if dev.type != "cuda":
        raise SkillshotError(f"VecSkillshotGame runs on a gfx950 GPU or the CPU backend, not {dev}")
    if not torch.cuda.is_available():
        raise SkillshotError("no GPU visible (use device='cpu' for libskillshot's CPU backend)")
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    return torch.device("cuda", idx)


class VecSkillshotGame:
    """N independent games (the reference SkillshotGame, batched).

    n_envs      games on this device
    env_offset  global id of game 0 (multi-GPU sharding; RNG is keyed by global id)
    seed        Philox key for random starts / random-policy actions
    tick_limit  episode length cap (SkillshotLearner.model_param_game_tick_limit, :62)
    random_positions  use random starts on reset (SkillshotLearner.use_random_start, :44)
    """

    def __init__(self, n_envs, device="cuda", seed=0, env_offset=0, tick_limit=2000,
                 random_positions=True, config=None):
        self.device = _resolve_device(device)
        self.is_cpu = self.device.type == "cpu"
        self.n = int(n_envs)
        if self.n <= 0:
            raise ValueError("n_envs must be > 0")
        self.seed = int(seed)
        self.env_offset = int(env_offset)
        self.tick_limit = int(tick_limit)
        self.random_positions = bool(random_positions)
        self._L = _capi.load()
        # one allocation, the planes back to back (88 B per game, every plane
        # 16-byte aligned): the multi-tick kernels address all six through
        # one buffer resource with 32-bit offsets (sk_env_step_multi)
        self._state_buf = torch.zeros(88 * self.n, dtype=torch.uint8, device=self.device)
        off = 0
        for name, dt, w in PLANES:
            nbytes = self.n * w * torch.empty((), dtype=dt).element_size()
            setattr(self, name, self._state_buf[off:off + nbytes].view(dt).view(self.n, w))
            off += nbytes
        view = _capi.SkStateView(self.n, *[getattr(self, name).data_ptr() for name, _, _ in PLANES])
        cfg = config if config is not None else _capi.default_config()
        self.config = cfg
        h = ctypes.c_void_p()
        self._sync()
        check(self._L.sk_env_attach(ctypes.byref(h), ctypes.byref(view), self.env_offset, self.seed,
                                    -1 if self.is_cpu else self.device.index, ctypes.byref(cfg)))
        self._h = h
        cp = ctypes.c_void_p()
        check(self._L.sk_env_counters_ptr(self._h, ctypes.byref(cp)))
        self._counters_ptr = cp.value
        self.reset(random_positions=False)

    # ------------------------------------------------------------------ utils
    def _stream(self):
        if self.is_cpu:
            return None
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _sync(self):
        if not self.is_cpu:
            torch.cuda.synchronize(self.device)

    def close(self):
        if getattr(self, "_h", None):
            self._sync()
            self._L.sk_env_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def step_counter(self):
        v = ctypes.c_uint64()
        check(self._L.sk_env_get_step_counter(self._h, ctypes.byref(v)))
        return v.value

    @step_counter.setter
    def step_counter(self, value):
        check(self._L.sk_env_set_step_counter(self._h, int(value)))

    def sync_step_counter(self, stream=None):
        """Stream-ordered: both device step slots take the current value and
        the host parity returns to 0.  Call it before capturing, before a
        graph replay, and after the last replay before the next eager call
        (a replay does not move the host parity): then replays and eager
        launches keep correct RNG keys in any mix (sk_env_sync_step_counter)."""
        check(self._L.sk_env_sync_step_counter(self._h, stream if stream is not None else self._stream()))

    def state_dict(self):
        """Host copy of the state planes (engine layout) + RNG counter."""
        d = {name: getattr(self, name).cpu().numpy().copy() for name, _, _ in PLANES}
        d["step_counter"] = self.step_counter
        return d

    def load_state_dict(self, d):
        self._sync()
        for name, dt, w in PLANES:
            src = torch.as_tensor(np.asarray(d[name]).reshape(self.n, w)).to(dt)
            getattr(self, name).copy_(src)
        if "step_counter" in d:
            self.step_counter = int(d["step_counter"])
        self._sync()

    def get_board(self, index=0):
        """SkillshotGame.get_board (SkillshotGame.py:36-56) of game `index`:
        int64 [250, 250], [x, y] indexing (host rasteriser, visualisation only)."""
        from .game import rasterize_board
        i = int(index)
        pos = self.pos[i].cpu().tolist()
        qpos = self.qpos[i].cpu().tolist()
        rot = self.rot[i].cpu().tolist()
        flags = int(self.misc[i, 1].item()) & 0xFFFFFFFF
        return rasterize_board(np.zeros((250, 250), dtype=np.int64), [pos[0:2], pos[2:4]], rot,
                               [qpos[0:2], qpos[2:4]], [flags & 0xFF, (flags >> 8) & 0xFF])

    def _board_out(self, m, out):
        shape = (m, self.config.board_w, self.config.board_h)
        if out is None:
            return torch.empty(shape, dtype=torch.uint8, device=self.device)
        if (out.dtype != torch.uint8 or out.device != self.device or tuple(out.shape) != shape or
                not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous uint8 tensor {shape} on {self.device}")
        return out

    def render(self, ids=None, out=None):
        """SkillshotGame.get_board (SkillshotGame.py:36-56) of many games in
        one launch (sk_env_render) on torch's current stream: uint8
        [M, board_w, board_h], [x, y] indexing, values 0..4 (get_board stays
        the reference's int64 host view of one game).  ids: None (every game,
        M = n_envs), a Python / numpy sequence of game indices (checked here:
        IndexError outside [0, n_envs)) or an int64 tensor on this device
        (not checked: an index out of range gives an all-zero board); any
        order, repeats allowed.  out: a contiguous uint8 [M, W, H] tensor on
        this device, 16-byte aligned.  Cells off the board are clipped and an
        invalid projectile is not drawn."""
        if ids is None:
            idx, m = None, self.n
        elif torch.is_tensor(ids):
            if ids.dtype != torch.int64 or ids.device != self.device or ids.dim() != 1:
                raise ValueError(f"ids must be a 1-d int64 tensor on {self.device}")
            idx, m = ids.contiguous(), ids.numel()
        else:
            a = np.asarray(ids)
            if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
                raise ValueError("ids must be a 1-d sequence of integers")
            a = a.astype(np.int64)
            if a.size and (a.min() < 0 or a.max() >= self.n):
                raise IndexError(f"game index out of range [0, {self.n})")
            idx, m = torch.from_numpy(a).to(self.device), a.size
        o = self._board_out(m, out)
        if m:
            check(self._L.sk_env_render(self._h, _ptr(idx), m, _ptr(o), self._stream()))
        return o

    def render_states(self, planes, out=None):
        """`render` of caller-owned states (sk_render_states), e.g. one game's
        recorded trace: planes maps every PLANES name to a tensor [L, width]
        on this device in the engine's layout; returns uint8 [L, W, H], one
        launch."""
        ts = []
        for name, dt, w in PLANES:
            t = torch.as_tensor(planes[name])
            if t.device != self.device:
                raise ValueError(f"plane {name} must be on {self.device}")
            ts.append(t.to(dt).reshape(-1, w).contiguous())
        m = ts[0].shape[0]
        if any(t.shape[0] != m for t in ts):
            raise ValueError("planes must hold the same number of states")
        o = self._board_out(m, out)
        if m:
            view = _capi.SkStateView(m, *[t.data_ptr() for t in ts])
            check(self._L.sk_render_states(ctypes.byref(self.config), -1 if self.is_cpu else self.device.index,
                                           ctypes.byref(view), None, m, _ptr(o), self._stream()))
        return o

    def trace_game(self, start_planes_row, actions):
        """One game's states after each tick of a recorded episode: the game
        starts from start_planes_row (every PLANES name -> its row of one
        game, [width]) and acts on actions float32 [L, 2, 2] (tick, player,
        {speed, look}), replayed on a one-game CPU-backend env with this env's
        config and tick limit and no auto-reset; the replay stops when the
        game ends.  Returns planes {name: [T, width]}, T <= L, on this env's
        device.  Exact: the CPU backend's step equals the device step bit
        for bit, and the device's multi-tick launches equal its per-tick
        step."""
        acts = torch.as_tensor(actions).detach().to("cpu", torch.float32).reshape(-1, 2, 1, 2)
        g = getattr(self, "_trace_env", None)
        if g is None:
            g = self._trace_env = VecSkillshotGame(1, device="cpu", seed=self.seed, tick_limit=self.tick_limit,
                                                   random_positions=False, config=self.config)
        g.tick_limit = self.tick_limit
        g.load_state_dict({name: torch.as_tensor(start_planes_row[name]).detach().cpu().numpy()
                           for name, _, _ in PLANES})
        rec = {name: [] for name, _, _ in PLANES}
        for a in acts:
            done = g.step(a, obs=False, auto_reset=False)["done"]
            for name, _, _ in PLANES:
                rec[name].append(getattr(g, name)[0].clone())
            if bool(done[0]):
                break
        return {name: (torch.stack(rec[name]) if rec[name] else torch.empty((0, w), dtype=dt)).to(self.device)
                for name, dt, w in PLANES}

    # convenience decoded views -------------------------------------------
    @property
    def ticks(self):
        return self.misc[:, 0]

    @property
    def flags(self):
        return self.misc[:, 1]

    @property
    def game_live(self):
        return ((self.misc[:, 1] >> 16) & 0xFF).to(torch.bool)

    @property
    def winner_id(self):
        return ((self.misc[:, 1] >> 24) & 0xFF).to(torch.uint8)

    @property
    def projectile_valid(self):
        f = self.misc[:, 1]
        return torch.stack([(f & 0xFF), (f >> 8) & 0xFF], -1).to(torch.bool)

    def counters(self, stream=None):
        """Episode counters (dones, hits by id, tick sum) accumulated on device
        by the step kernels' wavefront ballots (read on `stream`, default
        torch's current one: pass the stream the steps ran on)."""
        c = _capi.SkCounters()
        check(self._L.sk_env_read_counters(self._h, ctypes.byref(c), stream if stream is not None else self._stream()))
        return dict(dones=c.dones, hits_p1=c.hits_p1, hits_p2=c.hits_p2, ticks_sum=c.ticks_sum)

    def clear_counters(self, stream=None):
        """Zero the episode counters, ordered on `stream` (default torch's
        current one: pass the stream the steps run on)."""
        check(self._L.sk_env_clear_counters(self._h, stream if stream is not None else self._stream()))

    # ------------------------------------------------------------ reference API
    def reset(self, mask=None, random_positions=None):
        """SkillshotGame.game_reset (SkillshotGame.py:168-169) for masked envs."""
        rp = self.random_positions if random_positions is None else bool(random_positions)
        m = None if mask is None else self._u8(mask)
        check(self._L.sk_env_reset(self._h, _ptr(m), int(rp), self._stream()))

    def move_direction(self, player_id, speeds):
        """Player.move_direction_float (Player.py:57-68) for one player of every env."""
        v, s = self._f64_or_scalar(speeds)
        check(self._L.sk_player_move_direction(self._h, int(player_id), _ptr(v), s, self._stream()))

    def move_look(self, player_id, angles):
        """Player.move_look_float (Player.py:33-39)."""
        v, s = self._f64_or_scalar(angles)
        check(self._L.sk_player_move_look(self._h, int(player_id), _ptr(v), s, self._stream()))

    def move_discrete(self, player_id, kind, mask=None):
        """Keyboard moves (Player.py:27-55): kind 0 forwards, 1 backwards, 2 look left, 3 look right."""
        m = None if mask is None else self._u8(mask)
        check(self._L.sk_player_move_discrete(self._h, int(player_id), int(kind), _ptr(m), self._stream()))

    def shoot(self, player_id, mask=None):
        """Player.move_shoot_projectile (Player.py:78-89) for masked envs."""
        m = None if mask is None else self._u8(mask)
        check(self._L.sk_player_shoot(self._h, int(player_id), _ptr(m), self._stream()))

    def projectile_move(self, player_id, tick=True, mask=None):
        """Projectile.tick (Projectile.py:49-53) or, with tick=False, move_forwards (:38-47)."""
        m = None if mask is None else self._u8(mask)
        check(self._L.sk_projectile_move(self._h, int(player_id), int(bool(tick)), _ptr(m), self._stream()))

    def check_collision(self, hit_out=None):
        """SkillshotGame.check_collision (SkillshotGame.py:58-94); returns u8[N] id of the player hit (0 = none)."""
        h = hit_out if hit_out is not None else torch.empty(self.n, dtype=torch.uint8, device=self.device)
        check(self._L.sk_game_check_collision(self._h, _ptr(h), self._stream()))
        return h

    def game_tick(self):
        """SkillshotGame.game_tick (SkillshotGame.py:115-122)."""
        check(self._L.sk_game_tick(self._h, self._stream()))

    def features(self, out=None):
        """get_state() numerics (SkillshotGame.py:136-166): float64 [N, 2, 18] in FEATURE_KEYS order."""
        f = out if out is not None else torch.empty((self.n, 2, 18), dtype=torch.float64, device=self.device)
        check(self._L.sk_env_features(self._h, _ptr(f), self._stream()))
        return f

    def observe(self, reward="looking", obs_out=None, reward_out=None):
        """prepare_states (SkillshotLearner.py:512-543) -> obs [2,N,12] f32 and
        calculate_rewards_<reward> (:575-603) -> reward [2,N] f32 of the current state."""
        obs = obs_out if obs_out is not None else self.new_obs()
        rew = reward_out if reward_out is not None else torch.empty((2, self.n), dtype=torch.float32,
                                                                      device=self.device)
        check(self._L.sk_env_observe(self._h, _ptr(obs), _ptr(rew), REWARD_KINDS[reward], self._stream()))
        return obs, rew

    # ---------------------------------------------------------------- hot path
    def new_obs(self):
        return torch.empty((2, self.n, 12), dtype=torch.float32, device=self.device)

    def step(self, actions, obs=True, reward="looking", auto_reset=True, reset_obs=False, out=None):
        """One learner tick for every env (SkillshotLearner.py:302-324), one launch.

        actions: float32 [2, N, 2] (player, env, {speed, look}).
        Returns dict(obs [2,N,12] | None, reward [2,N] | None, done u8[N], winner u8[N],
        obs_reset [2,N,12] | None): obs/reward/done/winner describe the post-tick
        (terminal) state; with auto_reset the done envs are then reset and
        obs_reset holds the obs the next tick acts on.
        """
        a = self._actions(actions)
        o = out or {}
        obs_t = (o.get("obs") if o.get("obs") is not None else self.new_obs()) if obs else None
        rew_t = (o.get("reward") if o.get("reward") is not None else
                 torch.empty((2, self.n), dtype=torch.float32, device=self.device)) if obs else None
        done = o.get("done") if o.get("done") is not None else torch.empty(self.n, dtype=torch.uint8,
                                                                            device=self.device)
        win = o.get("winner") if o.get("winner") is not None else torch.empty(self.n, dtype=torch.uint8,
                                                                               device=self.device)
        obs_r = (o.get("obs_reset") if o.get("obs_reset") is not None else self.new_obs()) if reset_obs else None
        check(self._L.sk_env_step(self._h, _ptr(a), _ptr(obs_t), _ptr(rew_t), REWARD_KINDS[reward], _ptr(done),
                                  _ptr(win), self.tick_limit, int(bool(auto_reset)), int(self.random_positions),
                                  _ptr(obs_r), self._stream()))
        return dict(obs=obs_t, reward=rew_t, done=done, winner=win, obs_reset=obs_r)

    def step_insert(self, actions, acting_obs, ring, reward="looking", auto_reset=True, reset_obs=True, out=None,
                    total_copy=None):
        """`step` (obs and reward on) and the replay ring's insert of the tick's
        2N transitions (acting_obs[r], actions[r], reward[r], obs[r],
        done[r % N]) in ONE launch (sk_env_step_insert): equal, bit for bit,
        to step(...) followed by ring.add_dev(acting_obs, actions, reward,
        obs, done).  ring: learner.ReplayRing on this env's device;
        total_copy: an int64 element that receives the new row count too."""
        a = self._actions(actions)
        o = out or {}
        obs_t = o.get("obs") if o.get("obs") is not None else self.new_obs()
        rew_t = o.get("reward") if o.get("reward") is not None else torch.empty((2, self.n), dtype=torch.float32,
                                                                                device=self.device)
        done = o.get("done") if o.get("done") is not None else torch.empty(self.n, dtype=torch.uint8,
                                                                            device=self.device)
        win = o.get("winner") if o.get("winner") is not None else torch.empty(self.n, dtype=torch.uint8,
                                                                               device=self.device)
        obs_r = (o.get("obs_reset") if o.get("obs_reset") is not None else self.new_obs()) if reset_obs else None
        s = acting_obs.float().contiguous()
        if s.numel() != 2 * self.n * 12:
            raise ValueError("acting_obs must hold [2, N, 12] floats")
        check(self._L.sk_env_step_insert(self._h, _ptr(a), _ptr(obs_t), _ptr(rew_t), REWARD_KINDS[reward],
                                         _ptr(done), _ptr(win), self.tick_limit, int(bool(auto_reset)),
                                         int(self.random_positions), _ptr(obs_r), _ptr(s), _ptr(ring.buf), ring.cap,
                                         _ptr(ring.total_t), _ptr(ring.arrivals()), _ptr(total_copy),
                                         self._stream()))
        ring.total += 2 * self.n  # host mirror (exact while the row count is fixed)
        return dict(obs=obs_t, reward=rew_t, done=done, winner=win, obs_reset=obs_r)

    def _out_buf(self, o, key, shape, dtype):
        """o[key], checked (contiguous `dtype` `shape` on this device), or a new tensor when `o` has none"""
        t = o.get(key)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=self.device)
        elif tuple(t.shape) != shape or t.dtype != dtype or t.device != self.device or not t.is_contiguous():
            raise ValueError(f"out[{key!r}] must be contiguous {dtype} {shape} on {self.device}")
        return t

    def _act_step_out(self, o, acting_obs, actions, reset_obs, ring, total_copy):
        """what act_step and act_step_pool share: the dict they return (the
        tick's outputs, taken from `o` where it has them), the acting rows as
        the launch reads them and the ring's five C arguments"""
        obs_t = o.get("obs") if o.get("obs") is not None else self.new_obs()
        rew_t = o.get("reward") if o.get("reward") is not None else torch.empty((2, self.n), dtype=torch.float32,
                                                                                device=self.device)
        done = o.get("done") if o.get("done") is not None else torch.empty(self.n, dtype=torch.uint8,
                                                                            device=self.device)
        win = o.get("winner") if o.get("winner") is not None else torch.empty(self.n, dtype=torch.uint8,
                                                                               device=self.device)
        obs_r = (o.get("obs_reset") if o.get("obs_reset") is not None else self.new_obs()) if reset_obs else None
        act = actions if actions is not None else torch.empty((2, self.n, 2), dtype=torch.float32, device=self.device)
        s = acting_obs.float().contiguous()
        if s.numel() != 2 * self.n * 12 or act.numel() != 4 * self.n or not act.is_contiguous():
            raise ValueError("acting_obs must hold [2, N, 12] floats, actions [2, N, 2] (contiguous)")
        ring_args = ((_ptr(ring.buf), ring.cap, _ptr(ring.total_t), _ptr(ring.arrivals()), _ptr(total_copy))
                     if ring is not None else (None, 0, None, None, None))
        return dict(obs=obs_t, reward=rew_t, done=done, winner=win, obs_reset=obs_r, actions=act), s, ring_args

    def act_step(self, actor, acting_obs, noise_sd=0.0, action_sd=0.0, ring=None, reward="looking", auto_reset=True,
                 reset_obs=True, out=None, actions=None, total_copy=None, job=None):
        """The self-play tick's act + step (+ ring insert) in ONE launch
        (sk_env_act_step): `actor` (actor_kernel.ActorKernel32, the fp32
        actor) acts on acting_obs [2, N, 12] for both players of every game
        with parameter noise noise_sd and/or action noise action_sd, and the
        step runs on those actions; equal, bit for bit, to actor(...) with
        32-row tiles followed by step_insert (ring given; total_copy as
        step_insert's) or step.  job (_capi.SkStepJob): prepare the launch
        into it instead (sk_env_act_step_job; run by the actor step's
        backward launch, update_kernel.actor_step(step_job=job)).  Returns
        step's dict plus `actions` [2, N, 2]."""
        res, s, ring_args = self._act_step_out(out or {}, acting_obs, actions, reset_obs, ring, total_copy)
        pack = actor.ensure_pack()
        args = (self._h, _ptr(actor.flat), _ptr(pack), _ptr(s), _ptr(res["actions"]), float(noise_sd),
                float(action_sd), actor.seed, _ptr(actor._ctr), _ptr(res["obs"]), _ptr(res["reward"]),
                REWARD_KINDS[reward], _ptr(res["done"]), _ptr(res["winner"]), self.tick_limit, int(bool(auto_reset)),
                int(self.random_positions), _ptr(res["obs_reset"]), *ring_args)
        if job is not None:
            check(self._L.sk_env_act_step_job(*args, ctypes.byref(job)))
        else:
            check(self._L.sk_env_act_step(*args, self._stream()))
        if ring is not None:
            ring.total += 2 * self.n  # host mirror
        return res

    def act_episode(self, actor, start_obs, n_ticks=None, noise_sd=0.0, action_sd=0.0, reward="looking",
                    out=None):
        """The reference rule's episode collection in ONE launch
        (sk_env_act_episode; SkillshotLearner.model_train :289-318 for every
        game): from the current state every game plays until it ends (hit or
        tick limit), acting with `actor` (ActorKernel32) with fresh noise per
        tick.  start_obs [2, N, 12]: the observation of the current state.
        Returns dict(states [T+1, 2, N, 12], actions [T, 2, N, 2], rewards
        [T, 2, N], lengths int32 [N]); rows t < lengths[i] are game i's
        episode.  T = n_ticks (default: the tick limit); a game still live
        after T ticks continues in the next call (from states[T]).  The
        device step counter and the actor's noise call number (actor.calls)
        advance on device by max(lengths), the ticks the per-tick loop would
        have run."""
        T = int(self.tick_limit if n_ticks is None else n_ticks)
        o = out or {}
        st = o.get("states")
        if st is None or st.shape[0] < T + 1:
            st = torch.empty((T + 1, 2, self.n, 12), dtype=torch.float32, device=self.device)
        ac = o.get("actions")
        if ac is None or ac.shape[0] < T:
            ac = torch.empty((T, 2, self.n, 2), dtype=torch.float32, device=self.device)
        rw = o.get("rewards")
        if rw is None or rw.shape[0] < T:
            rw = torch.empty((T, 2, self.n), dtype=torch.float32, device=self.device)
        ln = o.get("lengths")
        if ln is None:
            ln = torch.empty(self.n, dtype=torch.int32, device=self.device)
        st[0].copy_(start_obs.reshape(2, self.n, 12))
        pack = actor.ensure_pack()
        check(self._L.sk_env_act_episode(self._h, _ptr(actor.flat), _ptr(pack), _ptr(st), _ptr(ac), _ptr(rw),
                                         _ptr(ln), T, float(noise_sd), float(action_sd), actor.seed,
                                         _ptr(actor._ctr), REWARD_KINDS[reward], self.tick_limit, self._stream()))
        return dict(states=st[:T + 1], actions=ac[:T], rewards=rw[:T], lengths=ln)

    def _seating(self, what, actors, pairs, block, o):
        """act_league's / act_step_pool's host check of a seating: (actors,
        the pairs as a tuple of int pairs, block).  `pairs` that is the very
        tuple an earlier call checked and returned (o["tables"][1], `o` that
        call's dict) for as many actors is taken as checked: a per-tick
        caller does not walk thousands of pairs again."""
        actors = list(actors)
        block = int(block)
        known = o.get("tables")
        if (known is not None and pairs is known[1] and len(known[0]) == len(actors) and
                len(pairs) * block == self.n and block > 0 and block % 32 == 0):
            return actors, pairs, block
        try:
            plist = tuple((int(i), int(j)) for i, j in pairs)
        except (TypeError, ValueError):
            raise ValueError("pairs must be a list of (seat-1 actor, seat-2 actor) index pairs")
        if not actors or not plist:
            raise ValueError(f"{what} needs at least one actor and one pairing")
        if not all(isinstance(a, ScriptedActor) or (hasattr(a, "flat") and hasattr(a, "ensure_pack")) for a in actors):
            raise TypeError("actors must be ActorKernel32 objects (the fp32 actor with its split pack) or "
                            "ScriptedActors")
        if block <= 0 or block % 32:
            raise ValueError("block must be a positive multiple of 32")
        if len(plist) * block != self.n:
            raise ValueError(f"the env holds {self.n} games, not len(pairs) * block = {len(plist) * block}")
        for i, j in plist:
            if not (0 <= i < len(actors) and 0 <= j < len(actors)):
                raise ValueError(f"pair ({i}, {j}) names an actor outside [0, {len(actors)})")
        return actors, plist, block

    def _seating_tables(self, actors, plist, o):
        """the two device tables of a seating (the actors' addresses, the
        pairs), taken from the dict `o` of an earlier call and uploaded only
        when the actors' buffers or the pairs differ from that call's:
        (nets, pairs, the key to keep as `tables`).  A ScriptedActor's row is
        (0, its kind code): the _bots symbols read it as a scripted seat."""
        addr = tuple((0, a.kind) if isinstance(a, ScriptedActor) else (a.flat.data_ptr(), a.ensure_pack().data_ptr())
                     for a in actors)
        nets = self._out_buf(o, "nets", (len(actors), 2), torch.int64)
        prs = self._out_buf(o, "pairs", (len(plist), 2), torch.int32)
        if o.get("tables") != (addr, plist) or nets is not o.get("nets") or prs is not o.get("pairs"):
            nets.copy_(torch.tensor(addr, dtype=torch.int64))
            prs.copy_(torch.tensor(plist, dtype=torch.int32))
        return nets, prs, (addr, plist)

    def _match_record(self, record, blocks, block, resume):
        """the MatchRecord of a recording act_match / act_league call (None
        for record None / 0): an int allocates one of that many rows per block
        of `block` games and tick_limit + 1 slabs, a MatchRecord is checked
        against the call and reused; without resume it starts at slab 0"""
        if record is None or (isinstance(record, int) and not isinstance(record, bool) and record == 0):
            return None
        from .record import MatchRecord
        if isinstance(record, MatchRecord):
            rec = record
        else:
            if isinstance(record, bool) or not isinstance(record, (int, np.integer)):
                raise TypeError("record must be None, a number of games per block or a MatchRecord")
            per = int(record)
            if not 1 <= per <= block:
                raise ValueError(f"record must lie in [1, {block}], the games of a block")
            games = (torch.arange(blocks)[:, None] * block + torch.arange(per)[None, :]).reshape(-1)
            rec = MatchRecord.allocate(self.tick_limit + 1, games, self.config, self.device, per_block=per)
        if not 1 <= rec.per_block <= block:
            raise ValueError(f"the record keeps {rec.per_block} games per block, a block has {block}")
        rec.check_layout(blocks * rec.per_block, self.device)
        if not resume:
            rec.ticks_run = 0
        return rec

    def _match_launch(self, what, plain, recording, seats, blocks, block, start_obs, n_ticks, reward, o, resume,
                      record, stats=None):
        """act_match's / act_league's launch over `blocks` blocks of `block`
        games: the C symbol `plain`, or `recording` (plain's arguments and the
        record) while the record has slabs left, with the seating's arguments
        `seats` between the handle and the shared ones.  stats (a buffer of
        new_stats): sk_env_act_league_stats instead, which takes the buffer
        and the record or NULL.  Returns act_match's dict."""
        if resume and (o.get("returns") is None or o.get("lengths") is None):
            raise ValueError(f"resume needs the dict a previous {what} returned as out")
        T = int(self.tick_limit if n_ticks is None else n_ticks)
        start = start_obs.reshape(2, self.n, 12)  # (may be out["obs"]: read before it is rewritten)
        obs2 = self._out_buf(o, "obs2", (2, 2, self.n, 12), torch.float32)
        ret = self._out_buf(o, "returns", (2, self.n), torch.float32)
        call_ln = self._out_buf(o, "call_lengths", (self.n,), torch.int32)
        total = self._out_buf(o, "lengths", (self.n,), torch.int32)
        obs = self._out_buf(o, "obs", (2, self.n, 12), torch.float32)
        obs2[0].copy_(start)
        if not resume:
            ret.zero_()
        rec = self._match_record(record, blocks, block, resume)
        T_rec = min(T, rec.slabs - 1 - rec.ticks_run) if rec is not None else 0
        outs = (_ptr(obs2), _ptr(ret), _ptr(call_ln), _ptr(o.get("last_half")))
        if stats is not None:
            st = rec.c_struct(rec.ticks_run) if T_rec >= 1 else None
            check(self._L.sk_env_act_league_stats(self._h, *seats, *outs, T_rec if st is not None else T,
                                                  REWARD_KINDS[reward], self.tick_limit, _ptr(stats),
                                                  ctypes.byref(st) if st is not None else None, self._stream()))
            if st is not None:
                rec.ticks_run += T_rec
        elif T_rec >= 1:
            st = rec.c_struct(rec.ticks_run)
            check(recording(self._h, *seats, *outs, T_rec, REWARD_KINDS[reward], self.tick_limit, ctypes.byref(st),
                            self._stream()))
            rec.ticks_run += T_rec
        else:
            check(plain(self._h, *seats, *outs, T, REWARD_KINDS[reward], self.tick_limit, self._stream()))
        torch.where((call_ln & 1).bool()[None, :, None], obs2[1], obs2[0], out=obs)
        if resume:
            total += call_ln
        else:
            total.copy_(call_ln)
        res = dict(lengths=total, returns=ret, obs=obs, obs2=obs2, call_lengths=call_ln,
                   last_half=o.get("last_half"))
        if stats is not None:
            res["stats"] = stats
        if rec is not None:
            torch.index_select(total, 0, rec.games, out=rec.lengths)
            res["record"] = rec
        return res

    def act_match(self, actor1, actor2, start_obs, n_ticks=None, reward="looking", out=None, resume=False,
                  record=None):
        """Two actors play every game head to head in ONE launch
        (sk_env_act_match; the loop of SkillshotLearner.py:302-318 with two
        policies): seat 1 (player id 1) acts from actor1, seat 2 from actor2
        (both ActorKernel32), without exploration noise, until each game ends
        (hit or tick limit) or n_ticks ticks (default: the tick limit) have
        run.  start_obs [2, N, 12]: the observation of the current state.
        Returns dict(lengths int32 [N], the ticks each game played; returns
        [2, N], each player's fp32 reward sum in tick order; obs [2, N, 12],
        every game's newest observation — of its final state once it has
        ended — plus the launch's buffers).  An ended game is not stepped
        again, so the env's planes hold the final states: winner_id is the id
        of the player who was HIT.  A game still live after n_ticks continues
        with act_match(..., start_obs=prev["obs"], out=prev, resume=True):
        lengths and returns then carry on from `prev` (the sums equal one
        long launch's, bit for bit).  out without resume only reuses the
        buffers.  The device step counter advances by max(lengths of this
        call); neither actor's noise call number moves.  Any N >= 1.

        record: keep what the first games did at every tick (record.py,
        sk_env_act_match_rec: the same launch, a few more stores per tick).
        An int r records games 0 .. r - 1 into a new MatchRecord of
        tick_limit + 1 slabs, returned as out["record"]; a MatchRecord is
        reused.  With resume=True the record continues at the slab the earlier
        calls' ticks reached (record.ticks_run), and its lengths follow
        out["lengths"].  A recording call runs no more ticks than the record
        has slabs left for; once they are used up the call runs unrecorded."""
        if self.is_cpu:
            raise SkillshotError("act_match runs on the GPU backend (SkillshotLearner.evaluate loops on the CPU one)")
        seats = (_ptr(actor1.flat), _ptr(actor1.ensure_pack()), _ptr(actor2.flat), _ptr(actor2.ensure_pack()))
        return self._match_launch("act_match", self._L.sk_env_act_match, self._L.sk_env_act_match_rec, seats, 1,
                                  self.n, start_obs, n_ticks, reward, out or {}, resume, record)

    def act_league(self, actors, pairs, block, start_obs, n_ticks=None, reward="looking", out=None, resume=False,
                   record=None, stats=False):
        """Every pairing of a league in ONE launch (sk_env_act_league):
        the env holds len(pairs) blocks of `block` games (a multiple of 32),
        and the games of block p play act_match's match with seat 1 acting
        from actors[pairs[p][0]] and seat 2 from actors[pairs[p][1]] (`actors`
        a list of ActorKernel32, `pairs` a host list of (i, j)).  A pairing
        that needs fewer than `block` games is padded by the caller with games
        that are not live: they are not stepped and their lengths are 0.
        start_obs, n_ticks, reward, resume, the step counter and the returned
        dict: act_match's.  The two device tables (the actors' addresses, the
        pairs) are kept in the returned dict (`nets`, `pairs`) and uploaded
        again only when the actors' buffers or `pairs` differ from the call
        that made them, so a repeated or captured call with out= allocates
        and uploads nothing.  record: act_match's, per pairing — an int r
        records the first r games of every block (row p r + k = game k of
        pairing p; the record's `pairs` names each row's pairing); a pairing
        the kernel's guard refuses and the pad games record nothing.
        `actors` may hold ScriptedActors (scripted.py): their seats run no
        forward, the launch (sk_env_act_league_bots) computes the policy on
        each tick's state itself and a record keeps the policy's actions; a
        list of nets alone goes through sk_env_act_league as before.
        stats=True: the launch (sk_env_act_league_stats, nets and scripted
        seats alike) also tallies what each seat did over the ticks its game
        lived (include/skillshot.h, csrc/sk_stats.hpp): the returned dict
        gains `stats`, the raw int32 [SK_N_STATS + 2, 2, N] buffer of
        new_stats (out["stats"] is initialised again and reused), whose words
        stats_tick before every step of the per-tick loop would have counted.
        The tallies are one call's, so stats does not combine with resume;
        every other entry is what the call without stats returns."""
        if self.is_cpu:
            raise SkillshotError("act_league runs on the GPU backend (SkillshotLearner.league loops on the CPU one)")
        if stats and resume:
            raise ValueError("act_league(stats=True) tallies one call's ticks: it does not combine with resume")
        o = out or {}
        actors, plist, block = self._seating("act_league", actors, pairs, block, o)
        nets, prs, tables = self._seating_tables(actors, plist, o)
        seats = (_ptr(nets), len(actors), _ptr(prs), len(plist), block)
        bots = any(isinstance(a, ScriptedActor) for a in actors)
        res = self._match_launch("act_league", self._L.sk_env_act_league_bots if bots else self._L.sk_env_act_league,
                                 self._L.sk_env_act_league_bots_rec if bots else self._L.sk_env_act_league_rec, seats,
                                 len(plist), block, start_obs, n_ticks, reward, o, resume, record,
                                 stats=self.new_stats(out=o.get("stats")) if stats else None)
        res.update(nets=nets, pairs=prs, tables=tables)
        if "record" in res:
            res["record"].pairs = [plist[p] for p in range(len(plist)) for _ in range(res["record"].per_block)]
        return res

    def act_step_pool(self, actors, pairs, block, acting_obs, noisy=None, noise_sd=0.0, action_sd=0.0, ring=None,
                      reward="looking", auto_reset=True, reset_obs=True, out=None, actions=None, total_copy=None):
        """The opponent-pool training tick in ONE launch
        (sk_env_act_step_pool): act_step's tick with act_league's seating.
        The env holds len(pairs) blocks of `block` games (a multiple of 32);
        in block p seat 1 acts from actors[pairs[p][0]] and seat 2 from
        actors[pairs[p][1]] (`actors` a list of ActorKernel32, `pairs` a host
        list of (i, j)).  `noisy` (an index into actors, or None) is the
        learner: its seats draw parameter noise noise_sd and / or action
        noise action_sd with that actor's seed and noise call number, which
        the launch advances; every other actor acts deterministically and
        its call number stays.  Equal, bit for bit, to every seated actor's
        forward (32-row tiles) on acting_obs [2, N, 12], each (seat, block)
        taking its actor's rows, followed by step_insert (ring given: all 2N
        transitions enter it; total_copy as step_insert's) or step.  The two
        device tables are kept in the returned dict (`nets`, `pairs`) and
        uploaded again only when the actors' buffers or `pairs` differ from
        the call that made them (out=); a per-tick caller passes the checked
        pairs back as well (pairs=out["tables"][1]) and skips the host's walk
        over them.  `actors` may hold ScriptedActors (scripted.py; never
        the noisy one): their seats act by the policy on the tick's state,
        in the same launch (sk_env_act_step_pool_bots), equal to
        bot_actions' rows in the composition above.  Returns act_step's
        dict."""
        if self.is_cpu:
            raise SkillshotError("act_step_pool runs on the GPU backend (SkillshotLearner.train_vs loops on the CPU one)")
        o = out or {}
        actors, plist, block = self._seating("act_step_pool", actors, pairs, block, o)
        if noisy is not None and (isinstance(noisy, bool) or not 0 <= int(noisy) < len(actors)):
            raise ValueError(f"noisy must be None or an actor index in [0, {len(actors)})")
        if noisy is None and (noise_sd != 0.0 or action_sd != 0.0):
            raise ValueError("noise_sd / action_sd need the noisy actor's index")
        if noisy is not None and isinstance(actors[int(noisy)], ScriptedActor):
            raise ValueError("the noisy actor must be a net, not a ScriptedActor")
        bots = any(isinstance(a, ScriptedActor) for a in actors)
        nets, prs, tables = self._seating_tables(actors, plist, o)
        res, s, ring_args = self._act_step_out(o, acting_obs, actions, reset_obs, ring, total_copy)
        learner = actors[int(noisy)] if noisy is not None else None
        check((self._L.sk_env_act_step_pool_bots if bots else self._L.sk_env_act_step_pool)(
            self._h, _ptr(nets), len(actors), _ptr(prs), len(plist), block, -1 if noisy is None else int(noisy),
            _ptr(s), _ptr(res["actions"]), float(noise_sd), float(action_sd),
            learner.seed if learner is not None else 0, _ptr(learner._ctr) if learner is not None else None,
            _ptr(res["obs"]), _ptr(res["reward"]), REWARD_KINDS[reward], _ptr(res["done"]), _ptr(res["winner"]),
            self.tick_limit, int(bool(auto_reset)), int(self.random_positions), _ptr(res["obs_reset"]), *ring_args,
            self._stream()))
        if ring is not None:
            ring.total += 2 * self.n  # host mirror
        res.update(nets=nets, pairs=prs, tables=tables)
        return res

    def step_raw(self, actions_ptr, done_ptr=None, obs_ptr=None, reward_ptr=None, winner_ptr=None,
                 auto_reset=True, stream=None):
        """Pointer-level fused step (bench / graph capture; no allocation)."""
        check(self._L.sk_env_step(self._h, actions_ptr, obs_ptr, reward_ptr, 0, done_ptr, winner_ptr,
                                  self.tick_limit, int(bool(auto_reset)), int(self.random_positions), None,
                                  stream if stream is not None else self._stream()))

    def step_multi(self, actions, n_ticks=None, slab0=0, done=None, winner=None, record=False, auto_reset=True,
                   stream=None):
        """n_ticks step-only learner ticks (SkillshotLearner.py:302-318: do_actions x2,
        game_tick, done, random restart) in ONE launch (sk_env_step_multi).

        actions: float32 [R, 2, N, 2], a ring of R per-tick slabs; tick t acts on
        slab (slab0 + t) % R.  n_ticks defaults to R.  done / winner: u8 [N]
        (the last tick's) or, with record=True, [n_ticks, N] (every tick's).
        Equal bit for bit to n_ticks `step(actions[s], obs=False)` calls."""
        a = torch.as_tensor(actions, device=self.device)
        if a.dtype != torch.float32 or not a.is_contiguous() or a.dim() != 4 or tuple(a.shape[1:]) != (2, self.n, 2):
            raise ValueError(f"actions must be contiguous float32 [R, 2, {self.n}, 2]")
        R = a.shape[0]
        T = R if n_ticks is None else int(n_ticks)
        rows = T if record else 1
        if done is None:
            done = torch.empty((rows, self.n), dtype=torch.uint8, device=self.device)
        if winner is None:
            winner = torch.empty((rows, self.n), dtype=torch.uint8, device=self.device)
        for t in (done, winner):
            if t.numel() < rows * self.n or t.dtype != torch.uint8 or not t.is_contiguous():
                raise ValueError(f"done / winner must be contiguous uint8 with {rows} x {self.n} elements")
        check(self._L.sk_env_step_multi(self._h, _ptr(a), R, int(slab0) % R, T, _ptr(done), _ptr(winner),
                                        self.n if record else 0, self.tick_limit, int(bool(auto_reset)),
                                        int(self.random_positions), stream if stream is not None else self._stream()))
        return done.view(rows, self.n) if record else done.view(-1)[: self.n], \
            winner.view(rows, self.n) if record else winner.view(-1)[: self.n]

    def step_multi_obs(self, actions, n_ticks=None, slab0=0, out_slabs=None, out0=0, reward="looking",
                       auto_reset=True, out=None, stream=None):
        """n_ticks ticks of the FULL contract (SkillshotLearner.py:302-324 with
        the actions given: do_actions x2, game_tick, prepare_states and the
        reward of the post-tick state, done, random restart) in ONE launch
        (sk_env_step_multi_obs).

        actions: float32 [R, 2, N, 2], tick t acting on slab (slab0 + t) % R;
        tick t writes output slab (out0 + t) % out_slabs (out_slabs defaults to
        n_ticks: one slab per tick) of obs [S, 2, N, 12], reward [S, 2, N],
        done / winner [S, N].  Equal bit for bit to n_ticks
        `step(actions[s], obs=True, reward=reward)` calls."""
        a = torch.as_tensor(actions, device=self.device)
        if a.dtype != torch.float32 or not a.is_contiguous() or a.dim() != 4 or tuple(a.shape[1:]) != (2, self.n, 2):
            raise ValueError(f"actions must be contiguous float32 [R, 2, {self.n}, 2]")
        R = a.shape[0]
        T = R if n_ticks is None else int(n_ticks)
        S = T if out_slabs is None else int(out_slabs)
        if out is None:
            out = dict(obs=torch.empty((S, 2, self.n, 12), dtype=torch.float32, device=self.device),
                       reward=torch.empty((S, 2, self.n), dtype=torch.float32, device=self.device),
                       done=torch.empty((S, self.n), dtype=torch.uint8, device=self.device),
                       winner=torch.empty((S, self.n), dtype=torch.uint8, device=self.device))
        for k, shape in (("obs", (S, 2, self.n, 12)), ("reward", (S, 2, self.n)), ("done", (S, self.n)),
                         ("winner", (S, self.n))):
            t = out.get(k)
            if t is not None and (tuple(t.shape) != shape or not t.is_contiguous()):
                raise ValueError(f"{k} must be contiguous {shape}")
        check(self._L.sk_env_step_multi_obs(self._h, _ptr(a), R, int(slab0) % R, T, _ptr(out.get("obs")),
                                            _ptr(out.get("reward")), REWARD_KINDS[reward], _ptr(out.get("done")),
                                            _ptr(out.get("winner")), S, int(out0) % S, self.tick_limit,
                                            int(bool(auto_reset)), int(self.random_positions),
                                            stream if stream is not None else self._stream()))
        return out

    def step_multi_raw(self, actions_ptr, ring, slab0, n_ticks, done_ptr=None, winner_ptr=None, out_stride=0,
                       auto_reset=True, stream=None):
        """Pointer-level sk_env_step_multi (bench / graph capture; no allocation)."""
        check(self._L.sk_env_step_multi(self._h, actions_ptr, int(ring), int(slab0), int(n_ticks), done_ptr,
                                        winner_ptr, int(out_stride), self.tick_limit, int(bool(auto_reset)),
                                        int(self.random_positions), stream if stream is not None else self._stream()))

    def gen_random_actions(self, n_ticks, out=None):
        """Random-policy actions float32 [n_ticks, 2, N, 2] (config 2 synthetic input)."""
        a = out if out is not None else torch.empty((n_ticks, 2, self.n, 2), dtype=torch.float32,
                                                    device=self.device)
        check(self._L.sk_gen_random_actions(self._h, _ptr(a), int(n_ticks), self._stream()))
        return a

    def bot_actions(self, kind, out=None):
        """Both seats' actions float32 [2, N, 2] of the scripted actor `kind`
        (a name or code, scripted.py) on the current state, the random
        policy's at the current step counter (sk_env_bot_act): one small
        launch on the GPU backend, the host loop on the CPU one, the same
        floats from both.  Advances nothing."""
        a = out if out is not None else torch.empty((2, self.n, 2), dtype=torch.float32, device=self.device)
        if (tuple(a.shape) != (2, self.n, 2) or a.dtype != torch.float32 or a.device != self.device or
                not a.is_contiguous()):
            raise ValueError(f"out must be contiguous float32 [2, {self.n}, 2] on {self.device}")
        check(self._L.sk_env_bot_act(self._h, kind_code(kind), _ptr(a), self._stream()))
        return a

    def _stats_fit(self):
        if self.tick_limit * max(self.config.board_w, self.config.board_h) > 2 ** 31 - 1:
            raise ValueError("the match statistics are int32: tick_limit * max(board_w, board_h) must fit in it")

    def new_stats(self, out=None):
        """A match-statistics buffer, int32 [SK_N_STATS + 2, 2, N]
        (include/skillshot.h: plane _capi.STAT_NAMES.index(name), seat, game;
        the last two planes carry the previous position between stats_tick
        calls), initialised: zeros, `closest` at INT32_MAX, x_prev at
        INT32_MIN.  out: a buffer to initialise again instead."""
        self._stats_fit()
        s = self._stats_buf(out) if out is not None else torch.empty((_capi.SK_N_STATS + 2, 2, self.n),
                                                                     dtype=torch.int32, device=self.device)
        s.zero_()
        s[_capi.STAT_NAMES.index("closest")] = _capi.SK_STAT_FAR
        s[_capi.SK_N_STATS] = _capi.SK_STAT_NO_PREV
        return s

    def _stats_buf(self, s):
        shape = (_capi.SK_N_STATS + 2, 2, self.n)
        if (not torch.is_tensor(s) or tuple(s.shape) != shape or s.dtype != torch.int32 or s.device != self.device or
                not s.is_contiguous()):
            raise ValueError(f"stats must be contiguous int32 {shape} on {self.device} (new_stats)")
        return s

    def stats_tick(self, stats, alive):
        """One tick of the match statistics (sk_env_stats_tick,
        csrc/sk_stats.hpp) from the current state, to be called before the
        step: every game whose `alive` entry is set (the caller's loop test:
        live and ticks < tick_limit) updates both seats' words of `stats`
        (new_stats).  Both backends, the same integers from both; the
        one-launch act_league(stats=True) tallies the same.  Advances
        nothing."""
        self._stats_fit()
        mask = self._u8(alive)  # (held until the call has been issued: it may be a converted copy)
        check(self._L.sk_env_stats_tick(self._h, _ptr(mask), _ptr(self._stats_buf(stats)), self._stream()))
        return stats

    def rollout_random(self, n_ticks):
        """n_ticks random-policy ticks with auto-reset, one launch, state in registers."""
        check(self._L.sk_env_rollout_random(self._h, int(n_ticks), self.tick_limit, self._stream()))

    # ---------------------------------------------------------------- helpers
    def _u8(self, mask):
        m = torch.as_tensor(mask, device=self.device)
        if m.dtype != torch.uint8:
            m = m.to(torch.uint8)
        m = m.contiguous()
        if m.numel() != self.n:
            raise ValueError("mask must have n_envs elements")
        return m

    def _f64_or_scalar(self, x):
        if isinstance(x, (int, float)):
            return None, float(x)
        t = torch.as_tensor(x, device=self.device).to(torch.float64).contiguous()
        if t.numel() == 1:
            return None, float(t.item())
        if t.numel() != self.n:
            raise ValueError("need one value per env")
        return t, 0.0

    def _actions(self, actions):
        a = torch.as_tensor(actions, device=self.device)
        if a.dtype != torch.float32:
            a = a.to(torch.float32)
        a = a.contiguous()
        if tuple(a.shape) != (2, self.n, 2):
            raise ValueError(f"actions must be float32 [2, {self.n}, 2], got {tuple(a.shape)}")
        return a
