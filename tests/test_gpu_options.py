"""The switches that used to be read from the environment once per process are options (csrc/c_api.cpp): kc_init reads
them from KC_<NAME>, kc_get_option reports them, the launchers follow them, and a kc_init after kc_shutdown picks up
changed values.  One child process, so that the environment and the options of this one are left alone."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a valid value of every former environment-only switch (and KC_REPLAY), then other ones for the second kc_init
FIRST = {"KC_POLY_ROWS": "24", "KC_POLY2_XCD": "0", "KC_DOWN2_XCD": "0", "KC_H2N_TILED": "0", "KC_NT_FORCE": "0x100",
         "KC_TUNE_CAP": "4096", "KC_UPLOAD_RING": "0", "KC_RESIZE_TILE_W": "64", "KC_RESIZE_TILE_H": "8", "KC_REPLAY": "0"}
SECOND = {"KC_POLY_ROWS": "12", "KC_POLY2_XCD": "1", "KC_DOWN2_XCD": "1", "KC_H2N_TILED": "1", "KC_NT_FORCE": "-1",
          "KC_TUNE_CAP": "0", "KC_UPLOAD_RING": "1", "KC_RESIZE_TILE_W": "128", "KC_RESIZE_TILE_H": "16", "KC_REPLAY": "1"}

CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, "tests")
import kanter_core_amd as kc
from util import SEED_A, resize_source

first, second = json.loads(sys.argv[1]), json.loads(sys.argv[2])
src = [resize_source(SEED_A, 0, 2048, 2048)]
px = np.arange(64 * 64 * 4, dtype=np.uint32).astype(np.uint8).reshape(64, 64, 4)
COUNTERS = ["poly2_launches", "poly2_rows_12", "poly2_rows_24", "poly2_xcd_order"]


def run(env):
    os.environ.update(env)
    kc.init(0)
    opts = {k: kc.get_option(k[3:].lower()) for k in env}
    before = {n: kc.stats_counter(n) for n in COUNTERS}
    out = kc.resize_image(kc.SlotImage.from_planes(src), (256, 256), kc.ResizeFilter.Gaussian)
    out.materialize()
    seen = {n: kc.stats_counter(n) - before[n] for n in COUNTERS}
    plane = out.planes()[0]
    u8 = kc.SlotImage.from_u8(px).to_u8()
    kc.set_option("replay", 1)  # an initial value, not a gate: the setter overrides KC_REPLAY
    replay = kc.get_option("replay")
    kc.shutdown()
    return opts, seen, plane, u8, replay


o1, s1, p1, u1, r1 = run(first)
o2, s2, p2, u2, r2 = run(second)
print(json.dumps({"opts": [o1, o2], "seen": [s1, s2], "replay": [r1, r2], "same_plane": bool(np.array_equal(p1.view(np.uint32), p2.view(np.uint32))),
                  "same_u8": bool(np.array_equal(u1, px) and np.array_equal(u2, px))}))
"""


def test_env_switches_are_read_at_every_init():
    env = {k: v for k, v in os.environ.items() if k not in FIRST}
    r = subprocess.run([sys.executable, "-c", CHILD, json.dumps(FIRST), json.dumps(SECOND)], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    for opts, env_values in zip(res["opts"], (FIRST, SECOND)):
        assert opts == {k: int(v, 0) for k, v in env_values.items()}
    # resize_poly2_kernel (Gaussian 2048^2 -> 256^2): the band height and the band order each kc_init read
    assert res["seen"][0] == {"poly2_launches": 1, "poly2_rows_12": 0, "poly2_rows_24": 1, "poly2_xcd_order": 0}
    assert res["seen"][1] == {"poly2_launches": 1, "poly2_rows_12": 1, "poly2_rows_24": 0, "poly2_xcd_order": 1}
    assert res["replay"] == [1, 1]
    assert res["same_plane"] and res["same_u8"]  # what the switches say never changes a result
