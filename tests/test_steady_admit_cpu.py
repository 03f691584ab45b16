"""Host check of the packed split kernel's launch-long admission to its steady
loop (csrc/sk_range.hpp: admit_cfg / admit_player / admit_game over the
kernel's own pack_fits_* tests), compiled for the CPU
(tests/steady_admit_check.cpp): the predicate is inductive under the tick's
integer recurrence for every (qcd, qage) entry pair, every cooldown_max in
[0, 127] and a game dying at any tick or never; run out over 480 ticks, no
admitted entry leaves the packed form, rejected entries exist that do
((5, 251) at its fifth tick) and admitted ones that reach age 255 exactly
((5, 250)).  Once more under the address and undefined-behaviour sanitizers
(a stand-alone program: nothing is preloaded)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "steady_admit_check.cpp")


def _run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-O2", "-std=c++17"] + flags + ["-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr, r.stderr
    return {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split())}


@pytest.mark.parametrize("name,flags", [("plain", []),
                                        ("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])])
def test_admission_is_inductive(tmp_path, name, flags):
    f = _run(tmp_path, "steady_admit_check_" + name, flags)
    assert f["violations"] == 0
    assert f["induction"] > 128 * 2 * 20000  # every admitted (cdmax, qcd, qage, qvalid), live and not
    assert f["game_steps"] > 65536
    assert f["runs"] == 5 * 256 * 256
    assert f["admitted"] > 0 and f["reach_255"] > 0 and f["rejected_leave"] > 0
