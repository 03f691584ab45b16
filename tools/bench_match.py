"""Head-to-head matches: one sk_env_act_match launch (k_act_match32: two
actors, one per seat, every game to its end) against the per-tick loop built
from the launches that existed before it — sk_actor_forward_f32 for seat 1,
sk_actor_forward_f32 for seat 2, sk_env_step, and the loop's alive.any() host
read — on the same start states.

Per size (4,096 and 65,536 games, tick limit 200, random starts, two actors
whose output biases make them turn and move): `warm` untimed runs of each
path, then `reps` timed runs of each, alternating, every run from the restored
start state.  Both paths are timed on the host clock between device
synchronisations (the loop syncs every tick by construction); the launch also
on device events.  The figure is microseconds per tick of the longest game
(time / max lengths); the record carries the median, minimum and maximum of
the runs, and checks that both paths played the same matches.

Each size runs in a child process under its own time limit, and a child that
fails ends the run: nothing more is started on the device after it.

    python tools/bench_match.py [--sizes 4096,65536] [--reps 7] [--tick-limit 200] [--out FILE]

One JSON line per record on stdout (and appended to --out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def emit(rec, path):
    line = json.dumps(rec)
    print(line, flush=True)
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def actor(seed):
    import torch
    from skillshot_learning_amd.learner import Actor
    torch.manual_seed(seed)
    a = Actor()
    with torch.no_grad():
        a.l3.bias.copy_(0.5 * torch.randn(2, generator=torch.Generator().manual_seed(seed)))
    return a.cuda()


def spread(xs):
    return dict(median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3))


def bench_size(n, limit, reps, warm, out_path):
    import torch
    import skillshot_learning_amd as ssa
    from skillshot_learning_amd.actor_kernel import ActorKernel32
    dev = torch.device("cuda", 0)
    k1, k2 = ActorKernel32(actor(23)), ActorKernel32(actor(24))
    g = ssa.VecSkillshotGame(n, device=dev, seed=6, tick_limit=limit)
    g.step_counter = 0
    g.reset(random_positions=True)
    start = g._state_buf.clone()
    obs0 = g.observe()[0].clone()
    bufs = {}

    def restore():
        g._state_buf.copy_(start)
        g.step_counter = 0
        torch.cuda.synchronize()

    def match():
        restore()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        m = g.act_match(k1, k2, obs0, n_ticks=limit, out=bufs.get("m"))
        e1.record()
        torch.cuda.synchronize()
        host = time.perf_counter() - t0
        bufs["m"] = m
        return host * 1e6, e0.elapsed_time(e1) * 1e3, m["lengths"].clone(), g.winner_id.clone()

    def loop():
        restore()
        alive = torch.ones(n, dtype=torch.bool, device=dev)
        lengths = torch.zeros(n, dtype=torch.int32, device=dev)
        winner = torch.zeros(n, dtype=torch.uint8, device=dev)
        obs = obs0
        t0 = time.perf_counter()
        while bool(alive.any()):
            out = g.step(torch.stack((k1(obs[0]), k2(obs[1]))), obs=True, auto_reset=False)
            done = out["done"].bool()
            lengths += alive.int()
            winner = torch.where(alive & done, out["winner"], winner)
            alive = alive & ~done
            obs = out["obs"]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6, None, lengths, winner

    for _ in range(warm):
        match()
        loop()
    mh, me, lh = [], [], []
    same = True
    for _ in range(reps):
        a = match()
        b = loop()
        T = int(a[2].max())
        same = same and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
        mh.append(a[0] / T)
        me.append(a[1] / T)
        lh.append(b[0] / int(b[2].max()))
    w = a[3]
    emit(dict(kind="match_vs_loop", games=n, tick_limit=limit, reps=reps, warm=warm, longest_game_ticks=T,
              mean_ticks=round(float(a[2].float().mean()), 2),
              hits_seat1=int((w == 1).sum()), hits_seat2=int((w == 2).sum()), draws=int((w == 0).sum()),
              same_matches=bool(same),
              match_us_per_tick_host=spread(mh), match_us_per_tick_events=spread(me),
              loop_us_per_tick_host=spread(lh),
              loop_over_match=round(statistics.median(lh) / statistics.median(mh), 2),
              loop="2 x sk_actor_forward_f32 + sk_env_step + alive.any() per tick",
              device=torch.cuda.get_device_name(0)), out_path)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", default="4096,65536")
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--warm", type=int, default=2)
    p.add_argument("--tick-limit", type=int, default=200)
    p.add_argument("--timeout", type=int, default=240, help="seconds per size")
    p.add_argument("--out", default=None)
    p.add_argument("--one", type=int, default=0, help="(child) measure this size in this process")
    a = p.parse_args()
    if a.one:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_match.py needs the GPU: no number is reported without one")
        bench_size(a.one, a.tick_limit, a.reps, a.warm, a.out)
        return
    for n in (int(s) for s in a.sizes.split(",") if s):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", str(n), "--reps", str(a.reps), "--warm",
               str(a.warm), "--tick-limit", str(a.tick_limit)] + (["--out", a.out] if a.out else [])
        try:
            rc = subprocess.run(cmd, timeout=a.timeout).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit(f"{n} games: no result within {a.timeout} s; stopping")
        if rc != 0:
            raise SystemExit(f"{n} games: the measurement exited with {rc}; stopping")


if __name__ == "__main__":
    main()
