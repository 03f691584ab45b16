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


def _build(tmp_path):
    exe = str(tmp_path / "fast_step_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe,
                    os.path.join(ROOT, "tests", "fast_step_check.cpp"), "-lm"], check=True)
    return exe


def test_look_step_sweep(tmp_path):
    """A projectile fired this tick flies at rot + l * look_speed, whose fp32 sincos is the angle
    addition sktrig::sincos_add, bounded for |l * look_speed| <= pi/4 only.  For look speeds 0.25, 0.4,
    0.78, 0.8, 1.0, 1.5 and 3.0 and 4e6 random (rotation, look action) pairs each: every decision the
    engine takes from the fp32 path (the host's gate sktrig::look_fits_add and fast_step_delta's
    `safe`) equals the fp64 one.  The gate sits at the documented bound pi/4, so 0.8 and 1.0 are
    refused although the ungated path shows no wrong decision before 1.5 (a few hundred in 4e6 with
    this draw, whose look actions clamp to +-1 a fifth of the time; some 280,000 at 3.0): that the
    ungated count at 3.0 is not 0 shows the sweep can see the defect."""
    r = subprocess.run([_build(tmp_path), "look", "4000000"], capture_output=True, text=True)
    print(r.stdout)
    rows = {}
    for line in r.stdout.splitlines():
        f = dict(kv.split("=") for kv in line.split())
        rows[float(f["look"])] = f
    assert sorted(rows) == [0.25, 0.4, 0.78, 0.8, 1.0, 1.5, 3.0]
    for look, f in rows.items():
        assert int(f["n"]) == 4_000_000 and int(f["safe"]) > 3_900_000
        assert int(f["gate"]) == (look <= 0.7853981633974483), look
        assert int(f["wrong"]) == 0, (look, f)
        if int(f["gate"]):
            assert int(f["raw_wrong"]) == 0 and float(f["max_err"]) <= 3.0e-7, (look, f)  # half of SKT_ADD_ERR
    assert int(rows[3.0]["raw_wrong"]) > 10_000
    assert r.returncode == 0, r.stdout + r.stderr


def test_fast_decisions_equal_fp64(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe, "10000000"], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    fields = dict(kv.split("=") for kv in r.stdout.split())
    assert int(fields["mismatches"]) == 0
    assert int(fields["n"]) >= 10_000_000
    assert 0.0 < float(fields["fallback"]) < 1e-3
