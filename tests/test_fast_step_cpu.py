"""Host check of the fast decisions of the step-only split tick
(csrc/sk_trig.hpp: fast_move_delta / fast_step_delta on sincos_fast and
sincos_add), compiled for the CPU with the kernels' flags: over 1e7 random
cases and the adversarial ones (half-integer deltas and their neighbours, the
ends of the fast range, huge and special rotations, NaN / inf / -0.0 actions;
speeds 3 and 5) every decision the fast path calls safe — the move, the fired
projectile's step, the step of one in flight — gives the integer the fp64
expression gives, and fewer than 1e-3 of the random cases go to the exact
path (the expected share is a few 1e-5)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fast_decisions_equal_fp64(tmp_path):
    exe = str(tmp_path / "fast_step_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe,
                    os.path.join(ROOT, "tests", "fast_step_check.cpp"), "-lm"], check=True)
    r = subprocess.run([exe, "10000000"], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    fields = dict(kv.split("=") for kv in r.stdout.split())
    assert int(fields["mismatches"]) == 0
    assert int(fields["n"]) >= 10_000_000
    assert 0.0 < float(fields["fallback"]) < 1e-3
