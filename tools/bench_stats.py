"""Match statistics in the one-launch league: what tallying them costs.

Per game count N (default 4096, 65536; one pairing of N games, tick limit 200,
random starts, two nets whose output biases make them turn and move), in one
child process per N, for three legs (net against net, net against the chaser,
still against still), every path from the same start states, `warm` untimed
runs of each and then `reps` timed runs in alternation, on device events:

  bots     sk_env_act_league_bots: the launch without statistics (a scripted
           actor nobody is paired with is listed, so that the net-net leg runs
           k_act_league32_bots as well)
  stats    sk_env_act_league_stats: the same launch tallying the statistics
  record   sk_env_act_league_bots_rec with record = N: every game's full
           record, what host-side statistics would need

A launch is reported as microseconds per tick of its longest game and per
million game-ticks played.  `stats` and `bots` must play the same games: the
child checks lengths and returns for equality and fails otherwise.

Each child runs under its own time limit, and a child that fails ends the
run: nothing more is started on the device after it.

    python tools/bench_stats.py [--sizes 4096,65536] [--reps 7] [--out FILE]

One JSON line per record on stdout (and appended to --out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def emit(rec, path):
    line = json.dumps(rec)
    print(line, flush=True)
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def spread(xs):
    return dict(median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3))


def bench_size(n, limit, reps, warm, out_path):
    sys.path.insert(0, ROOT)
    import torch
    import skillshot_learning_amd as ssa
    from skillshot_learning_amd.actor_kernel import ActorKernel32
    from skillshot_learning_amd.learner import Actor
    from skillshot_learning_amd.vec_env import PLANES
    os.environ["SK_FWD16"] = "0"

    def actor(seed):  # bench_league's actors
        torch.manual_seed(seed)
        a = Actor()
        with torch.no_grad():
            a.l3.bias.copy_(0.5 * torch.randn(2, generator=torch.Generator().manual_seed(seed)))
        return a.cuda()

    nets = [actor(23), actor(24)]
    k0, k1 = (ActorKernel32(m, seed=5 + k) for k, m in enumerate(nets))
    Bot = ssa.ScriptedActor
    g = ssa.VecSkillshotGame(n, device="cuda", seed=6, tick_limit=limit)
    g.step_counter = 0
    g.reset(random_positions=True)
    start = {name: getattr(g, name).clone() for name, _, _ in PLANES}
    obs0 = g.observe()[0].clone()
    legs = {"net_net": [k0, k1, Bot("still")], "net_chaser": [k0, Bot("chaser")], "still_still": [Bot("still"), Bot("still")]}
    bufs, recs = {}, {}

    def run(leg, path):
        for name, t in start.items():
            getattr(g, name).copy_(t)
        g.step_counter = 1
        key = (leg, path)
        kw = {}
        if path == "stats":
            kw["stats"] = True
        elif path == "record":
            kw["record"] = recs.get(leg, n)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        m = g.act_league(legs[leg], [(0, 1)], n, obs0, n_ticks=limit, out=bufs.get(key), **kw)
        e1.record()
        torch.cuda.synchronize()
        if path == "record":
            recs[leg] = m.pop("record")
        bufs[key] = m
        us = e0.elapsed_time(e1) * 1e3
        T, played = int(m["lengths"].max()), int(m["lengths"].sum())
        return us / T, us / played * 1e6, T, played

    paths = ("bots", "stats", "record")
    for leg in legs:
        for _ in range(warm):
            for path in paths:
                run(leg, path)
        a, b = bufs[(leg, "bots")], bufs[(leg, "stats")]
        if not (torch.equal(a["lengths"], b["lengths"]) and torch.equal(a["returns"], b["returns"])):
            raise SystemExit(f"{leg}: the launch with statistics played other games")
        got = {path: [] for path in paths}
        for _ in range(reps):
            for path in paths:
                got[path].append(run(leg, path))
        rec = dict(kind="stats", leg=leg, games=n, tick_limit=limit, reps=reps, warm=warm,
                   device=torch.cuda.get_device_name(0), longest_game_ticks=got["bots"][0][2],
                   game_ticks=got["bots"][0][3])
        for path in paths:
            rec[path] = dict(us_per_tick=spread([r[0] for r in got[path]]),
                             us_per_million_game_ticks=spread([r[1] for r in got[path]]))
        emit(rec, out_path)
        recs.pop(leg, None)  # the full record of 65,536 games is large: one leg's at a time
        bufs.pop((leg, "record"), None)
        torch.cuda.empty_cache()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", default="4096,65536", help="games, comma separated (multiples of 32)")
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--warm", type=int, default=2)
    p.add_argument("--tick-limit", type=int, default=200)
    p.add_argument("--timeout", type=int, default=240, help="seconds per child")
    p.add_argument("--out", default=None)
    p.add_argument("--one", default="", help="(child) measure this game count in this process")
    a = p.parse_args()
    if a.one:
        sys.path.insert(0, ROOT)
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_stats.py needs the GPU: no number is reported without one")
        bench_size(int(a.one), a.tick_limit, a.reps, a.warm, a.out)
        return
    for size in (s for s in a.sizes.split(",") if s):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", size, "--reps", str(a.reps), "--warm", str(a.warm),
               "--tick-limit", str(a.tick_limit)] + (["--out", a.out] if a.out else [])
        try:
            rc = subprocess.run(cmd, timeout=a.timeout).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit(f"{size}: no result within {a.timeout} s; stopping")
        if rc != 0:
            raise SystemExit(f"{size}: the measurement exited with {rc}; stopping")


if __name__ == "__main__":
    main()
