"""Scripted actors in the one-launch kernels: what a seat without an MFMA tile
costs, and that the net-only launches are what they were.

Per game count N (default 4096, 65536; one pairing of N games, tick limit 200,
random starts, two nets whose output biases make them turn and move), in one
child process per N, every path from the same start states, `warm` untimed
runs of each and then `reps` timed runs in alternation, on device events:

  match        sk_env_act_match, net against net (two tiles per tick)
  league_net   sk_env_act_league, the same two nets (the net-only league)
  bot_<kind>   sk_env_act_league_bots, net against the scripted actor `kind`
               (one tile per tick), for still and chaser
  bots_only    sk_env_act_league_bots, chaser against aimer (no tile)
  pool_net     sk_env_act_step_pool, learner and one frozen net, per tick
  pool_bot     sk_env_act_step_pool_bots, learner and the chaser, per tick

A whole-match launch is reported as microseconds per tick of its longest game
and per million game-ticks played (a workgroup leaves once its 32 games have
ended, so launches whose games end early run fewer workgroups per tick; the
second figure divides that out).  The pool ticks are `ticks` eager launches
per run, microseconds per tick.

--parent DIR (a checkout of the parent revision with its library built) adds,
per N, `rounds` alternations of two more children that run the net-only paths
alone (match, league_net, pool_net: what the parent has), one importing the
package from this tree and one from DIR, so both revisions' net-only launches
are measured side by side doing the same work in the same order.

Each child runs under its own time limit, and a child that fails ends the
run: nothing more is started on the device after it.

    python tools/bench_bots.py [--sizes 4096,65536] [--reps 7] [--parent DIR] [--rounds 3] [--out FILE]

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


def bench_size(n, limit, reps, warm, ticks, tree, label, net_only, out_path):
    sys.path.insert(0, tree)
    import torch
    import skillshot_learning_amd as ssa
    from skillshot_learning_amd.actor_kernel import ActorKernel32
    from skillshot_learning_amd.learner import Actor, ReplayRing, pool_pairs
    from skillshot_learning_amd.vec_env import PLANES
    os.environ["SK_FWD16"] = "0"
    has_bots = not net_only

    def actor(seed):  # bench_league's actors
        torch.manual_seed(seed)
        a = Actor()
        with torch.no_grad():
            a.l3.bias.copy_(0.5 * torch.randn(2, generator=torch.Generator().manual_seed(seed)))
        return a.cuda()

    nets = [actor(23), actor(24)]
    k0, k1 = (ActorKernel32(m, seed=5 + k) for k, m in enumerate(nets))
    g = ssa.VecSkillshotGame(n, device="cuda", seed=6, tick_limit=limit)
    g.step_counter = 0
    g.reset(random_positions=True)
    start = {name: getattr(g, name).clone() for name, _, _ in PLANES}
    obs0 = g.observe()[0].clone()

    def rewind():
        for name, t in start.items():
            getattr(g, name).copy_(t)
        g.step_counter = 1

    bufs = {}

    def match_run(name, call):
        rewind()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        m = bufs[name] = call(bufs.get(name))
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3
        T, played = int(m["lengths"].max()), int(m["lengths"].sum())
        return us / T, us / played * 1e6, T, played

    paths = {"match": lambda o: g.act_match(k0, k1, obs0, n_ticks=limit, out=o),
             "league_net": lambda o: g.act_league([k0, k1], [(0, 1)], n, obs0, n_ticks=limit, out=o)}
    if has_bots:
        Bot = ssa.ScriptedActor
        for kind in ("still", "chaser"):
            paths["bot_" + kind] = lambda o, kind=kind: g.act_league([k0, Bot(kind)], [(0, 1)], n, obs0,
                                                                   n_ticks=limit, out=o)
        paths["bots_only"] = lambda o: g.act_league([Bot("chaser"), Bot("aimer")], [(0, 1)], n, obs0, n_ticks=limit,
                                                    out=o)

    # the pool tick: pool_pairs' seating of the learner and one opponent, parameter noise, a ring
    pairs = pool_pairs(n, 1)
    ring = ReplayRing(1 << 19, "cuda")
    pool_actors = {"pool_net": [k0, k1]}
    if has_bots:
        pool_actors["pool_bot"] = [k0, Bot("chaser")]
    pool_out = {}

    def pool_run(name):
        rewind()
        obs = [obs0.clone(), None]
        res = pool_out.get(name)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for t in range(ticks):
            o = dict(res) if res is not None else {}
            o["obs_reset"] = obs[(t + 1) & 1]
            res = g.act_step_pool(pool_actors[name], pairs if res is None else res["tables"][1], 32, obs[t & 1],
                                  noisy=0, noise_sd=0.5, ring=ring, out=o)
            obs[(t + 1) & 1] = res["obs_reset"]
        e1.record()
        torch.cuda.synchronize()
        pool_out[name] = res
        return e0.elapsed_time(e1) * 1e3 / ticks

    for _ in range(warm):
        for name, call in paths.items():
            match_run(name, call)
        for name in pool_actors:
            pool_run(name)
    got = {name: [] for name in list(paths) + list(pool_actors)}
    for _ in range(reps):
        for name, call in paths.items():
            got[name].append(match_run(name, call))
        for name in pool_actors:
            got[name].append(pool_run(name))
    rec = dict(kind="bots_net_only" if net_only else "bots", tree=label, games=n, tick_limit=limit, reps=reps, warm=warm, pool_ticks=ticks,
               device=torch.cuda.get_device_name(0))
    for name in paths:
        rec[name] = dict(us_per_tick=spread([r[0] for r in got[name]]),
                         us_per_million_game_ticks=spread([r[1] for r in got[name]]),
                         longest_game_ticks=got[name][0][2], game_ticks=got[name][0][3])
    for name in pool_actors:
        rec[name] = dict(us_per_tick=spread(got[name]))
    emit(rec, out_path)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", default="4096,65536", help="games, comma separated (multiples of 64)")
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--warm", type=int, default=2)
    p.add_argument("--ticks", type=int, default=100, help="pool ticks per timed run")
    p.add_argument("--tick-limit", type=int, default=200)
    p.add_argument("--timeout", type=int, default=240, help="seconds per child")
    p.add_argument("--parent", default=None, help="a checkout of the parent revision, its library built")
    p.add_argument("--rounds", type=int, default=3, help="alternations of this tree and --parent")
    p.add_argument("--out", default=None)
    p.add_argument("--one", default="", help="(child) measure this game count in this process")
    p.add_argument("--tree", default=ROOT, help="(child) import the package from this checkout")
    p.add_argument("--label", default="this")
    p.add_argument("--net-only", action="store_true", help="(child) the paths the parent revision has")
    a = p.parse_args()
    if a.one:
        sys.path.insert(0, a.tree)
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_bots.py needs the GPU: no number is reported without one")
        bench_size(int(a.one), a.tick_limit, a.reps, a.warm, a.ticks, a.tree, a.label, a.net_only, a.out)
        return
    for size in (s for s in a.sizes.split(",") if s):
        children = [("this", ROOT, False)]
        if a.parent:
            children += [("this", ROOT, True), ("parent", os.path.abspath(a.parent), True)] * a.rounds
        for label, tree, net_only in children:
            cmd = [sys.executable, os.path.abspath(__file__), "--one", size, "--tree", tree, "--label", label,
                   "--reps", str(a.reps), "--warm", str(a.warm), "--ticks", str(a.ticks), "--tick-limit",
                   str(a.tick_limit)] + (["--net-only"] if net_only else []) + (["--out", a.out] if a.out else [])
            try:
                rc = subprocess.run(cmd, timeout=a.timeout).returncode
            except subprocess.TimeoutExpired:
                raise SystemExit(f"{size} ({label}): no result within {a.timeout} s; stopping")
            if rc != 0:
                raise SystemExit(f"{size} ({label}): the measurement exited with {rc}; stopping")


if __name__ == "__main__":
    main()
