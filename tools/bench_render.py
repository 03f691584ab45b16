"""The batched board rasteriser's time (sk_env_render, csrc/sk_render.hip)
against the write floor for the same bytes, and model_train's board replay on
the on-device episode path against the per-tick loop.

Render: VecSkillshotGame.render() of every game's current state (a random
start played for 300 random-policy ticks) into a preallocated uint8
[N, 250, 250] tensor, N = 4,096 (256 MB) and 65,536 (4.1 GB).  Beside it
out.zero_() on the same tensor: the same bytes stored once with no
arithmetic.  Both on device events around `inner` back-to-back launches,
after warm-up, `reps` windows each, alternating; the record carries the
median and the minimum per launch and their ratio.  The expectation to
report against is render <= 1.5 x the fill.

Epoch (--epoch): one model_train(1, save_boards=True) epoch at 4,096 games,
host clock around the call with a device synchronise at both ends, after one
warm-up epoch, with SK_EPISODE_KERNEL=0 (the per-tick loop with a get_board
round trip per tick: the only path save_boards had before the renderer) and
with the default (episodes in act_episode launches, the boards from
trace_game + one render_states launch), and the latter without boards.
Writing the boards to disk is stubbed out.

    python tools/bench_render.py [--sizes 4096,65536] [--reps 7] [--epoch] [--tick-limit 200] [--out FILE]

One JSON line per record on stdout (and appended to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def emit(rec, path):
    line = json.dumps(rec)
    print(line, flush=True)
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def windows(fns, inner, reps, stream):
    """per-launch milliseconds of each fn: reps windows of `inner` launches, alternating"""
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(inner):
                fn()
            e1.record(stream)
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / inner)
    return times


def bench_render(n, reps, out_path):
    import skillshot_learning_amd as ssa
    dev = torch.device("cuda", 0)
    g = ssa.VecSkillshotGame(n, device=dev, seed=7, tick_limit=2000)
    g.reset(random_positions=True)
    g.rollout_random(300)
    out = torch.empty((n, 250, 250), dtype=torch.uint8, device=dev)
    nbytes = out.numel()
    inner = max(4, min(64, (1 << 32) // nbytes))  # about 4 GB stored per window
    fns = (lambda: g.render(out=out), lambda: out.zero_())
    for fn in fns:  # warm-up: code objects, allocator
        for _ in range(3):
            fn()
    g.render(out=out)
    nonzero = int((out != 0).sum()) if n <= 4096 else None  # the boards are not empty (the fill ran last above)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream(dev)
    t_render, t_fill = windows(fns, inner, reps, st)
    med_r, med_f = statistics.median(t_render), statistics.median(t_fill)
    emit(dict(kind="render_vs_fill", boards=n, bytes=nbytes, inner=inner, reps=reps,
              render_ms_median=round(med_r, 4), render_ms_min=round(min(t_render), 4),
              fill_ms_median=round(med_f, 4), fill_ms_min=round(min(t_fill), 4),
              render_tb_s=round(nbytes / med_r / 1e9, 3), fill_tb_s=round(nbytes / med_f / 1e9, 3),
              ratio_median=round(med_r / med_f, 3), ratio_min=round(min(t_render) / min(t_fill), 3),
              nonzero_cells=nonzero, device=torch.cuda.get_device_name(0)), out_path)
    del out, g
    torch.cuda.empty_cache()


def bench_epoch(n, tick_limit, out_path):
    from skillshot_learning_amd import learner
    for flag, boards, path in (("0", True, "per-tick loop, get_board per tick"),
                               ("1", True, "act_episode + trace_game + render_states"),
                               ("1", False, "act_episode, no boards")):
        os.environ["SK_EPISODE_KERNEL"] = flag
        L = learner.SkillshotLearner(n_envs=n, device="cuda", seed=3, tick_limit=tick_limit, precision="fp32")
        L.save_training_boards = lambda seqs: None
        secs = []
        for _ in range(2):  # the first epoch warms up (code objects, captured fit chunks, buffers)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            prog = L.model_train(1, save_boards=boards, board_game=0)
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        ticks = prog["epoch_ticks"][-1]
        emit(dict(kind="epoch", save_boards=boards, games=n, tick_limit=tick_limit, SK_EPISODE_KERNEL=flag, path=path,
                  warmup_epoch_s=round(secs[0], 3), epoch_s=round(secs[1], 3), max_ticks=int(ticks.max()),
                  board_game_ticks=int(ticks[0]), device=torch.cuda.get_device_name(0)), out_path)
        del L
        torch.cuda.empty_cache()
    os.environ.pop("SK_EPISODE_KERNEL", None)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", default="4096,65536")
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--epoch", action="store_true")
    p.add_argument("--epoch-games", type=int, default=4096)
    p.add_argument("--tick-limit", type=int, default=200)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_render.py needs the GPU: no number is reported without one")
    for n in (int(s) for s in a.sizes.split(",") if s):
        bench_render(n, a.reps, a.out)
    if a.epoch:
        bench_epoch(a.epoch_games, a.tick_limit, a.out)


if __name__ == "__main__":
    main()
