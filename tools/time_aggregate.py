"""Time mvs_sweep_aggregate (csrc/aggregate.hip) through mvs_profile_read(MVS_K_ARGMIN): the packed volume of a 4-view sweep of
synth.make_views with 128 planes, at 640 x 480 and 1920 x 1080, for 4 and 8 paths (P1 16, P2 128, cap 4080), after warm-up.  Beside every
time: the bytes the launch structure must move divided by 8 TB/s -- per cell 6 for the cost conversion (4 read, 2
written), 10 for the row launch (C read twice, S written once, then read and written), 6 per column launch (C read, S read and written)
and 6 for the selection (S and the packed cell read).  One JSON line per case; --out FILE also writes them as a JSON list.

    python tools/time_aggregate.py [--iters 10] [--out profiles/aggregate/time_aggregate.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mesh-reconstruction_amd", "python"))
import numpy as np  # noqa: E402,F401

import mvs_amd  # noqa: E402
from mvs_amd import synth  # noqa: E402

HBM_TBS = 8.0
PLANES, VIEWS = 128, 4


def bytes_per_cell(paths):
    return 6 + 10 + 6 * (paths - 2) + 6


def one(W, H, iters):
    main_cam, main_img, side_cams, sides, _ = synth.make_views(W, H, VIEWS, radius=0.3)
    recs = []
    with mvs_amd.Context(W, H) as ctx:
        ctx.sweep_set(main_cam, main_img, side_cams, sides, PLANES)
        ctx.sweep_run(0, VIEWS, mvs_amd.MVS_SWEEP_VOLUME)
        ctx.sweep_argmin()
        _, _, i_wta, _ = ctx.sweep_fetch()
        for paths in (4, 8):
            for _ in range(2):
                ctx.sweep_aggregate(paths)
            ctx.synchronize()
            ctx.profile_enable(True)
            ctx.profile_read(reset=True)
            for _ in range(iters):
                ctx.sweep_aggregate(paths)
            ms, n = ctx.profile_read(reset=True)
            ctx.profile_enable(False)
            _, _, i_agg, _ = ctx.sweep_fetch()
            t = ms[mvs_amd.MVS_K_ARGMIN] / max(n[mvs_amd.MVS_K_ARGMIN], 1)
            cells = W * H * PLANES
            floor_ms = cells * bytes_per_cell(paths) / (HBM_TBS * 1e12) * 1e3
            rec = {"size": "%dx%d" % (W, H), "planes": PLANES, "paths": paths, "iters": iters, "aggregate_ms": round(t, 4),
                   "bytes_per_cell": bytes_per_cell(paths), "bytes_floor_ms_at_8TBs": round(floor_ms, 4), "times_the_floor": round(t / floor_ms, 1),
                   "pixels_reselected": round(float(np.mean(i_agg != i_wta)), 4)}
            print(json.dumps(rec), flush=True)
            recs.append(rec)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    recs = []
    for W, H in ((640, 480), (1920, 1080)):
        recs += one(W, H, a.iters)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
