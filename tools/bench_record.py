"""Match records: what recording costs the one-launch match, and what the
one-launch record saves over the only way there was before it.

4,096 games, tick limit 200, random starts, tools/bench_match.py's two actors
and method: `warm` untimed and `reps` timed runs of every path, alternating in
one process, every run from the restored start state; microseconds per tick of
the longest game on the host clock between device synchronisations (and on
device events for the launches).  Paths:

  plain     act_match, no record (k_act_match32)
  rec_all   act_match recording every game (k_act_match32_rec)
  rec_32    act_match recording the first 32 games
  loop      the per-tick loop (two sk_actor_forward_f32, sk_env_step,
            alive.any()) cloning the live games' planes, actions and rewards
            into a record every tick: MatchRecord.loop_before / loop_after,
            what SK_MATCH_KERNEL=0 runs

Before timing, rec_all's record and loop's are compared once, bit for bit
(that one loop run with SK_FWD16=0, the match kernel's 32-row tiles).

--parent-root DIR (a checkout of the parent commit with its library built)
adds the second measurement: `plain` on this tree and on the parent's,
alternating run by run, each tree in a child process of its own that stays up
for the whole measurement (a library is chosen when the package is imported).

    python tools/bench_record.py [--games 4096] [--reps 7] [--tick-limit 200] [--parent-root DIR] [--out FILE]

One JSON line per record on stdout (and appended to --out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def setup(n, limit):
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

    def restore():
        g._state_buf.copy_(start)
        g.step_counter = 0
        torch.cuda.synchronize()

    return torch, dev, g, k1, k2, obs0, restore


def timed_match(torch, g, k1, k2, obs0, limit, restore, bufs, record=None):
    restore()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kw = {} if record is None else dict(record=record)
    t0 = time.perf_counter()
    e0.record()
    m = g.act_match(k1, k2, obs0, n_ticks=limit, out=bufs.get("m"), **kw)
    e1.record()
    torch.cuda.synchronize()
    host = time.perf_counter() - t0
    bufs["m"] = {k: v for k, v in m.items() if k != "record"}
    T = int(m["lengths"].max())
    return host * 1e6 / T, e0.elapsed_time(e1) * 1e3 / T, T


def bench_paths(n, limit, reps, warm, out_path):
    torch, dev, g, k1, k2, obs0, restore = setup(n, limit)
    from skillshot_learning_amd.record import MatchRecord
    bufs = {}
    recs = {"rec_all": MatchRecord.allocate(limit + 1, torch.arange(n), g.config, dev, per_block=n),
            "rec_32": MatchRecord.allocate(limit + 1, torch.arange(32), g.config, dev, per_block=32),
            "loop": MatchRecord.allocate(limit + 1, torch.arange(n), g.config, dev, per_block=n)}

    def loop():
        rec = recs["loop"]
        restore()
        alive = torch.ones(n, dtype=torch.bool, device=dev)
        lengths = torch.zeros(n, dtype=torch.int32, device=dev)
        obs, t = obs0, 0
        t0 = time.perf_counter()
        while bool(alive.any()):
            act = torch.stack((k1(obs[0]), k2(obs[1])))
            ar = rec.loop_before(g, t, alive)
            out = g.step(act, obs=True, auto_reset=False)
            rec.loop_after(g, t, ar, act, out["reward"], out["done"])
            lengths += alive.int()
            alive = alive & ~out["done"].bool()
            obs = out["obs"]
            t += 1
        rec.lengths.copy_(lengths)
        torch.cuda.synchronize()
        host = (time.perf_counter() - t0) * 1e6 / t
        return host, None, t

    paths = {"plain": lambda: timed_match(torch, g, k1, k2, obs0, limit, restore, bufs),
             "rec_all": lambda: timed_match(torch, g, k1, k2, obs0, limit, restore, bufs, recs["rec_all"]),
             "rec_32": lambda: timed_match(torch, g, k1, k2, obs0, limit, restore, bufs, recs["rec_32"]),
             "loop": loop}
    # the two ways to a full record, compared once, whole tensors bit for bit.  For this one run the loop's
    # forwards take the match kernel's 32-row tiles (SK_FWD16=0: the 16-row tiles they default to at this size
    # round differently in the last bits); the timed runs use the default, the loop at its fastest
    prev = os.environ.get("SK_FWD16")
    os.environ["SK_FWD16"] = "0"
    paths["rec_all"]()
    paths["loop"]()
    if prev is None:
        del os.environ["SK_FWD16"]
    else:
        os.environ["SK_FWD16"] = prev
    a, b = recs["rec_all"], recs["loop"]
    same = torch.equal(a.lengths, b.lengths)
    tensors = [(a.states[k], b.states[k]) for k in a.states] + [(a.actions, b.actions), (a.rewards, b.rewards)]
    for x, y in tensors:
        same = same and torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    if not same:
        raise SystemExit("the launch's record and the loop's differ: nothing is timed")
    for _ in range(warm):
        for f in paths.values():
            f()
    host = {k: [] for k in paths}
    events = {k: [] for k in paths}
    T = 0
    for _ in range(reps):
        for k, f in paths.items():
            h, e, T = f()
            host[k].append(h)
            if e is not None:
                events[k].append(e)
    ln = a.lengths.float()
    rec_bytes = sum(x.numel() * x.element_size() for x, _ in tensors)
    emit(dict(kind="record_paths", games=n, tick_limit=limit, reps=reps, warm=warm, longest_game_ticks=T,
              mean_ticks=round(float(ln.mean()), 2), records_equal=bool(same), full_record_bytes=rec_bytes,
              us_per_tick_host={k: spread(v) for k, v in host.items()},
              us_per_tick_events={k: spread(v) for k, v in events.items() if v},
              rec_all_over_plain=round(statistics.median(host["rec_all"]) / statistics.median(host["plain"]), 3),
              loop_over_rec_all=round(statistics.median(host["loop"]) / statistics.median(host["rec_all"]), 2),
              device=torch.cuda.get_device_name(0)), out_path)


def serve_plain(n, limit):
    """(child) one timed plain act_match per line read from stdin; the figures as one JSON line each"""
    torch, dev, g, k1, k2, obs0, restore = setup(n, limit)
    bufs = {}
    print(json.dumps(dict(ready=True)), flush=True)
    for line in sys.stdin:
        if line.strip() != "go":
            break
        h, e, T = timed_match(torch, g, k1, k2, obs0, limit, restore, bufs)
        print(json.dumps(dict(host=h, events=e, ticks=T)), flush=True)


def bench_trees(n, limit, reps, warm, parent_root, timeout, out_path):
    kids = {}
    try:
        for name, root in (("this", ROOT), ("parent", os.path.abspath(parent_root))):
            cmd = [sys.executable, os.path.abspath(__file__), "--serve-plain", "--games", str(n), "--tick-limit",
                   str(limit), "--root", root]
            kids[name] = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        deadline = time.time() + timeout

        def ask(k, msg):
            if msg:
                k.stdin.write(msg + "\n")
                k.stdin.flush()
            line = k.stdout.readline()
            if not line or time.time() > deadline:
                raise SystemExit("a tree's child process ended or ran out of time; stopping")
            return json.loads(line)

        for k in kids.values():
            ask(k, None)
        res = {name: dict(host=[], events=[]) for name in kids}
        ticks = {}
        for r in range(warm + reps):
            for name, k in kids.items():
                d = ask(k, "go")
                ticks[name] = d["ticks"]
                if r >= warm:
                    res[name]["host"].append(d["host"])
                    res[name]["events"].append(d["events"])
    finally:
        for k in kids.values():
            try:
                k.stdin.close()
                k.wait(timeout=30)
            except Exception:
                k.kill()
    emit(dict(kind="plain_this_tree_vs_parent", games=n, tick_limit=limit, reps=reps, warm=warm,
              longest_game_ticks=ticks,
              us_per_tick_host={k: spread(v["host"]) for k, v in res.items()},
              us_per_tick_events={k: spread(v["events"]) for k, v in res.items()}), out_path)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--games", type=int, default=4096)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--warm", type=int, default=2)
    p.add_argument("--tick-limit", type=int, default=200)
    p.add_argument("--timeout", type=int, default=300, help="seconds per measurement")
    p.add_argument("--parent-root", default=None)
    p.add_argument("--out", default=None)
    p.add_argument("--one", action="store_true", help="(child) the four paths in this process")
    p.add_argument("--serve-plain", action="store_true", help="(child) plain runs on request")
    p.add_argument("--root", default=ROOT, help="(child) the tree whose package is imported")
    a = p.parse_args()
    if a.one or a.serve_plain:
        sys.path.insert(0, a.root)
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_record.py needs the GPU: no number is reported without one")
        if a.one:
            bench_paths(a.games, a.tick_limit, a.reps, a.warm, a.out)
        else:
            serve_plain(a.games, a.tick_limit)
        return
    cmd = [sys.executable, os.path.abspath(__file__), "--one", "--games", str(a.games), "--reps", str(a.reps),
           "--warm", str(a.warm), "--tick-limit", str(a.tick_limit)] + (["--out", a.out] if a.out else [])
    try:
        rc = subprocess.run(cmd, timeout=a.timeout).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit(f"the paths: no result within {a.timeout} s; stopping")
    if rc != 0:
        raise SystemExit(f"the paths: the measurement exited with {rc}; stopping")
    if a.parent_root:
        bench_trees(a.games, a.tick_limit, a.reps, a.warm, a.parent_root, a.timeout, a.out)


if __name__ == "__main__":
    main()
