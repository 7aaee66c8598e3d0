"""Time mvs_sweep_window (csrc/window.hip) through mvs_profile_read(MVS_K_ARGMIN): the packed volume of a 4-view sweep of
synth.make_views with 128 planes, at 640 x 480 and 1920 x 1080, for radius 1, 2 and 4, tau 255 (the box) and 20 (gated by the main
image), with and without MVS_WINDOW_SELECT, after warm-up.  No time is fixed for this kernel; every time is reported against two
references: the bytes the pass must move divided by 8 TB/s -- 8 per cell (4 read, 4 written) and 13 per pixel (the guide read, the three
maps written) -- and the time of mvs_sweep_argmin on the same volume in the same run, an existing kernel that reads 4 bytes per cell once
(the window moves twice its bytes).  One JSON line per case; --out FILE also writes them as a JSON list.

    python tools/time_window.py [--iters 10] [--out profiles/window/times.json]
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


def timed(ctx, call, iters):
    for _ in range(2):
        call()
    ctx.synchronize()
    ctx.profile_enable(True)
    ctx.profile_read(reset=True)
    for _ in range(iters):
        call()
    ms, n = ctx.profile_read(reset=True)
    ctx.profile_enable(False)
    return ms[mvs_amd.MVS_K_ARGMIN] / max(n[mvs_amd.MVS_K_ARGMIN], 1)


def one(W, H, iters):
    main_cam, main_img, side_cams, sides, _ = synth.make_views(W, H, VIEWS, radius=0.3)
    recs = []
    with mvs_amd.Context(W, H) as ctx:
        ctx.sweep_set(main_cam, main_img, side_cams, sides, PLANES)
        ctx.sweep_run(0, VIEWS, mvs_amd.MVS_SWEEP_VOLUME)
        argmin_ms = timed(ctx, ctx.sweep_argmin, iters)
        _, _, i_wta, _ = ctx.sweep_fetch()
        pixels, cells = W * H, W * H * PLANES
        floor_ms = (8 * cells + 13 * pixels) / (HBM_TBS * 1e12) * 1e3
        for radius in (1, 2, 4):
            for tau in (255, 20):
                for select in (False, True):
                    t = timed(ctx, lambda: ctx.sweep_window(radius, tau, None, select=select), iters)
                    rec = {"size": "%dx%d" % (W, H), "planes": PLANES, "radius": radius, "tau": tau, "select": select, "iters": iters,
                           "window_ms": round(t, 4), "bytes_floor_ms_at_8TBs": round(floor_ms, 4), "times_the_floor": round(t / floor_ms, 1),
                           "argmin_ms": round(argmin_ms, 4), "times_argmin": round(t / argmin_ms, 1)}
                    if select:
                        rec["pixels_reselected"] = round(float(np.mean(ctx.sweep_fetch()[2] != i_wta)), 4)
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
