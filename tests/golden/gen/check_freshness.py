#!/usr/bin/env python3
"""The committed fixtures are what the committed generator produces (needs the reference tree, see refenv.py).

    python tests/golden/gen/check_freshness.py [section ...]        (default: func, which includes media and volfunc; `textured` adds the
                                                                     whole-kernel section, ~30 s; `settings` the sensor-settings
                                                                     matrix, tests/golden/settings_matrix.npz: 66 whole-kernel runs
                                                                     of the reference, measured 560 s on 8 cores - optional, never
                                                                     part of the default)

`gen_goldens.py --only <section>` draws every fixture's random inputs from a stream seeded by the fixture's file name, so a section
re-run must reproduce the committed arrays bit for bit.  Arrays are compared, not file bytes: the zip container stores timestamps.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)
GEN = os.path.join(HERE, "gen_goldens.py")
REPO = os.path.abspath(os.path.join(GOLD, "..", ".."))


def _regen(section, out):
    res = subprocess.run([sys.executable, GEN, "--only", section, "--out", out], capture_output=True, text=True, cwd=REPO)
    assert res.returncode == 0, res.stderr[-2000:]
    made = sorted(f for f in os.listdir(out) if f.endswith(".npz"))
    assert made, "the section wrote nothing"
    return made


def _same(a_path, b_path):
    a, b = np.load(a_path, allow_pickle=False), np.load(b_path, allow_pickle=False)
    assert sorted(a.files) == sorted(b.files), (a_path, set(a.files) ^ set(b.files))
    for k in a.files:
        x, y = a[k], b[k]
        assert x.dtype == y.dtype and x.shape == y.shape, (a_path, k)
        assert x.tobytes() == y.tobytes(), f"{os.path.basename(a_path)}[{k}] differs from what the generator writes now"


def check(section):
    with tempfile.TemporaryDirectory() as out:
        made = _regen(section, out)
        for f in made:
            _same(os.path.join(out, f), os.path.join(GOLD, f))
    print(f"{section}: {len(made)} fixtures reproduced")


if __name__ == "__main__":
    for s in sys.argv[1:] or ["func"]:
        check(s)
