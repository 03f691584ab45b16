"""Host check of csrc/sk_range.hpp (the packed split kernel's steady tick:
one-compare range tests and one collision test per lane of a pair), compiled
for the CPU: every unsigned interval form against hit_test_s's signed
expressions over all 256 x 256 byte pairs per axis (sizes 5 / 3, 1 and 255),
the move's and the projectile's bounds over every step the steady tick can
take, and 1e7 random full tuples oriented as lanes 0 and 1 hold them and
combined as the kernel does against collide_s: no mismatch, and every kind of
outcome met (player 1 only, player 2 only, both, neither, an overlapping
projectile that is invalid, a hit in a game that is not live).  Once more
under the address and undefined-behaviour sanitizers (a stand-alone program:
nothing is preloaded)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "pair_collision_check.cpp")


def _run(tmp_path, name, flags, n):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-O2", "-std=c++17"] + flags + ["-o", exe, SRC], check=True)
    r = subprocess.run([exe, str(n)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr, r.stderr
    return {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split())}


@pytest.mark.parametrize("name,flags,n", [("plain", [], 10_000_000),
                                          ("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
                                           10_000_000)])
def test_pair_collision_equals_collide_s(tmp_path, name, flags, n):
    f = _run(tmp_path, "pair_collision_check_" + name, flags, n)
    assert f["mismatches"] == 0
    assert f["n"] >= 10_000_000
    assert f["exhaustive"] >= 5 * 65536
    for k in ("h1_only", "h2_only", "both", "neither", "invalid_overlap", "dead_hit"):
        assert f[k] > 0, k
