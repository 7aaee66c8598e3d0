"""Time the depth-map filter (csrc/depth_filter.hip), in one process, after warm-up.

The synthetic scene with 4 views at 640 x 480 and 1920 x 1080, swept over 128 planes and refined; the input of every filter call is the
context's own depth map.  Per size: the median stage, the mean stage and both, at radius 1..4, without a guide (tau = 255) and gated by
the staged main image (tau = 16), the depth gate at 8 plane steps; and mvs_sweep_argmin over the 128 planes on the same context as the
yardstick (a pass that reads the whole volume once).  All are HIP-event times of the launches (mvs_profile_read: MVS_K_ARGMIN), one
reading per iteration.  The variants are timed in turn and the whole turn is repeated --passes times, so that a drift of the machine
falls on all of them: the figure is the median of passes x iters readings with the minimum and maximum beside it.  bytes_floor is what a
stage has to move at least: the map read once and written once, the guide read once when it is gated; both stages move twice that.
One JSON line per size; --out FILE writes the list.

    python tools/time_depth_filter.py [--iters 10] [--passes 2] [--out profiles/depth_filter/times.json]
"""
import argparse
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mesh-reconstruction_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402,F401  (the HIP runtime first)

import mvs_amd  # noqa: E402
from mvs_amd import synth  # noqa: E402
from time_band import kernel_ms, spread  # noqa: E402

PLANES, VIEWS, MAX_STEPS, TAU = 128, 4, 8.0, 16
SIZES = ((640, 480), (1920, 1080))
STAGES = (("median", True, False), ("mean", False, True), ("both", True, True))
ARGMIN = (mvs_amd.MVS_K_ARGMIN,)


def one(W, H, iters, passes):
    main_cam, main_img, side_cams, sides, _ = synth.make_views(W, H, VIEWS)
    rec = {"case": "synthetic scene", "size": "%dx%d" % (W, H), "planes": PLANES, "views": VIEWS, "max_step_in_plane_steps": MAX_STEPS, "gated_tau": TAU,
           "iters": iters, "passes": passes, "date": datetime.date.today().isoformat()}
    step = MAX_STEPS * 2.0 / PLANES
    with mvs_amd.Context(W, H) as ctx:
        rec["device"] = ctx.info()
        ctx.sweep_set(main_cam, main_img, side_cams, sides, PLANES)
        ctx.sweep_run(0, VIEWS, mvs_amd.MVS_SWEEP_VOLUME | mvs_amd.MVS_SWEEP_FUSED_ARGMIN)
        ctx.sweep_refine_depth()
        depth = ctx.sweep_result_pointers()[0]

        def call(radius, tau, median, mean):
            return lambda: ctx.depth_filter(depth, radius, tau, step, None, median, mean, fetch=False)

        variants = [("argmin_%d_planes" % PLANES, ctx.sweep_argmin, 0)]
        for radius in (1, 2, 3, 4):
            for tag, tau in (("", 255), ("_gated", TAU)):
                for name, median, mean in STAGES:
                    floor = W * H * (8 + (1 if tau < 255 else 0)) * (2 if median and mean else 1)
                    variants.append(("%s_r%d%s" % (name, radius, tag), call(radius, tau, median, mean), floor))
        ms = {key: [] for key, _, _ in variants}
        for _ in range(passes):
            for key, fn, _ in variants:
                ms[key] += kernel_ms(ctx, fn, iters, ARGMIN)
        yardstick = spread(ms[variants[0][0]])["median"]
        for key, _, floor in variants:
            s = spread(ms[key])
            rec[key] = {"ms": s, "over_argmin": round(s["median"] / yardstick, 3)}
            if floor:
                rec[key].update(bytes_floor=floor, ns_per_pixel=round(s["median"] * 1e6 / (W * H), 4), floor_GB_per_s=round(floor / (s["median"] * 1e6), 1))
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    recs = [one(W, H, a.iters, a.passes) for W, H in SIZES]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
