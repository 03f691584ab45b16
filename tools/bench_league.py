"""League evaluation: SkillshotLearner.league's one launch (sk_env_act_league,
k_act_league32: every ordered pairing of K actors side by side) against the
way the same table was obtained before it — the K (K - 1) / 2 pairwise
SkillshotLearner.evaluate(opponent, swap_sides=True) calls, each two
sk_env_act_match launches — from the same start states.

Per size "K:games" (default 8:1024, 4:4096, 16:256; tick limit 200, random
starts, K actors whose output biases make them turn and move, one small
learner per actor so that evaluate(opponent=learner_j) copies no weights):
`warm` untimed runs of each path, then `reps` timed runs of each, alternating.
Both are timed on the host clock between device synchronisations, whole calls
(start states, launches, tallies, the host read); the league's launch
(act_league: its copies, the kernel, the counter launch) also on device
events, reported as microseconds per tick of the longest game.  The record
carries the median, minimum and maximum of the runs and checks that both
paths return the same tallies.

Each size runs in a child process under its own time limit, and a child that
fails ends the run: nothing more is started on the device after it.

    python tools/bench_league.py [--sizes 8:1024,4:4096,16:256] [--reps 7] [--tick-limit 200] [--out FILE]

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
    return a


def spread(xs):
    return dict(median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3))


def bench_size(K, games, limit, reps, warm, out_path):
    import torch
    from skillshot_learning_amd.learner import SkillshotLearner
    from skillshot_learning_amd.vec_env import VecSkillshotGame
    os.environ["SK_FWD16"] = "0"
    learners = []
    for k in range(K):  # bench_match's actors 23, 24, then on
        L = SkillshotLearner(n_envs=32, device="cuda", seed=3, tick_limit=limit, replay_capacity=1024,
                             precision="fp32")
        with torch.no_grad():
            L.model_actor.load_state_dict(actor(23 + k).state_dict())
        learners.append(L)
    seed = 6
    launch = {}
    plain = VecSkillshotGame.act_league

    def timed_act_league(self, *a, **kw):  # the launch inside league(), on device events
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        m = plain(self, *a, **kw)
        e1.record()
        launch.update(e0=e0, e1=e1, m=m)
        return m

    VecSkillshotGame.act_league = timed_act_league

    def league():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = learners[0].league([None] + learners[1:], games=games, tick_limit=limit, seed=seed)
        torch.cuda.synchronize()
        host = time.perf_counter() - t0
        T = int(launch["m"]["lengths"].max())
        return host * 1e3, launch["e0"].elapsed_time(launch["e1"]) * 1e3 / T, T, r

    def pairwise():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = {}
        for i in range(K):
            for j in range(i + 1, K):
                res[(i, j)] = learners[i].evaluate(opponent=learners[j], games=games, swap_sides=True,
                                                   tick_limit=limit, seed=seed)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, res

    def same(r, res):
        for (i, j), e in res.items():
            a, b = e["legs"]
            if (r["seat_wins"][i][j], r["seat_losses"][i][j], r["seat_draws"][i][j], r["mean_ticks"][i][j]) != \
                    (a["wins"], a["losses"], a["draws"], a["mean_ticks"]):
                return False
            if (r["seat_wins"][j][i], r["seat_losses"][j][i], r["seat_draws"][j][i], r["mean_ticks"][j][i]) != \
                    (b["losses"], b["wins"], b["draws"], b["mean_ticks"]):
                return False
        return True

    for _ in range(warm):
        league()
        pairwise()
    lh, lt, ph = [], [], []
    ok = True
    for _ in range(reps):
        a = league()
        b = pairwise()
        ok = ok and same(a[3], b[1])
        lh.append(a[0])
        lt.append(a[1])
        ph.append(b[0])
    r = a[3]
    P, block = K * (K - 1), 32 * ((games + 31) // 32)
    emit(dict(kind="league_vs_pairwise", actors=K, games_per_pairing=games, pairings=P, league_games=P * block,
              tick_limit=limit, reps=reps, warm=warm, longest_game_ticks=a[2],
              hits=sum(map(sum, r["seat_wins"])) + sum(map(sum, r["seat_losses"])),
              draws=sum(map(sum, r["seat_draws"])), same_tallies=bool(ok),
              league_ms_host=spread(lh), league_launch_us_per_tick_events=spread(lt),
              pairwise_ms_host=spread(ph),
              pairwise_over_league=round(statistics.median(ph) / statistics.median(lh), 2),
              league_beats_pairwise_by_more_than_the_spread=bool(max(lh) < min(ph)),
              pairwise=f"{P // 2} x evaluate(opponent, swap_sides=True) = {P} sk_env_act_match launches",
              device=torch.cuda.get_device_name(0)), out_path)
    if not ok:
        raise SystemExit("the two paths returned different tallies")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", default="8:1024,4:4096,16:256", help="K:games per ordered pairing, comma separated")
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--warm", type=int, default=2)
    p.add_argument("--tick-limit", type=int, default=200)
    p.add_argument("--timeout", type=int, default=240, help="seconds per size")
    p.add_argument("--out", default=None)
    p.add_argument("--one", default="", help="(child) measure this K:games in this process")
    a = p.parse_args()
    if a.one:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_league.py needs the GPU: no number is reported without one")
        K, games = (int(x) for x in a.one.split(":"))
        bench_size(K, games, a.tick_limit, a.reps, a.warm, a.out)
        return
    for size in (s for s in a.sizes.split(",") if s):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", size, "--reps", str(a.reps), "--warm",
               str(a.warm), "--tick-limit", str(a.tick_limit)] + (["--out", a.out] if a.out else [])
        try:
            rc = subprocess.run(cmd, timeout=a.timeout).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit(f"{size}: no result within {a.timeout} s; stopping")
        if rc != 0:
            raise SystemExit(f"{size}: the measurement exited with {rc}; stopping")


if __name__ == "__main__":
    main()
