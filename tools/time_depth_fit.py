"""Time the depth-map plane fit (csrc/depth_fit.hip), in one process, after warm-up.

The synthetic scene with 4 views at 640 x 480 and 1920 x 1080, swept over 128 planes and refined; the input of every call is the
context's own depth map.  Per size: mvs_depth_fit at radius 1..4, without a guide (tau = 255) and gated by the staged main image
(tau = 30), the depth gate at 8 plane steps; beside each, in the same turn, mvs_depth_filter with the mean stage alone at the same radius
and gate -- the existing kernel with the same staging and window walk, and so the yardstick; mvs_depth_fit_normals; and
mvs_propagate_init (ZNCC, radius 2) with and without recorded slopes.  All are HIP-event times of the call's launches (mvs_profile_read:
MVS_K_ARGMIN, MVS_K_FUSE, MVS_K_SWEEP), one reading per call: 5 warm-up calls, then the median of 20 readings with the minimum and the
maximum beside it.  bytes_floor is what a fit has to move at least: the map read once, four maps and the members written once, the
guide read once when it is gated.  One JSON line per size; --out FILE writes the list.

    python tools/time_depth_fit.py [--iters 20] [--warmup 5] [--out profiles/depth_fit/times.json]
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
from time_band import spread  # noqa: E402

PLANES, VIEWS, MAX_STEPS, TAU = 128, 4, 8.0, 30
SIZES = ((640, 480), (1920, 1080))


def event_ms(ctx, call, kinds, iters, warmup):
    for _ in range(warmup):
        call()
    ctx.synchronize()
    ctx.profile_enable(True)
    ctx.profile_read(reset=True)
    out = []
    for _ in range(iters):
        call()
        ms, _ = ctx.profile_read(reset=True)
        out.append(float(sum(ms[k] for k in kinds)))
    ctx.profile_enable(False)
    return out


def one(W, H, iters, warmup):
    main_cam, main_img, side_cams, sides, _ = synth.make_views(W, H, VIEWS)
    rec = {"case": "synthetic scene", "size": "%dx%d" % (W, H), "planes": PLANES, "views": VIEWS, "max_step_in_plane_steps": MAX_STEPS, "gated_tau": TAU,
           "iters": iters, "warmup": warmup, "date": datetime.date.today().isoformat()}
    step = MAX_STEPS * 2.0 / PLANES
    with mvs_amd.Context(W, H) as ctx:
        rec["device"] = ctx.info()
        ctx.sweep_set(main_cam, main_img, side_cams, sides, PLANES)
        ctx.sweep_run(0, VIEWS, mvs_amd.MVS_SWEEP_VOLUME | mvs_amd.MVS_SWEEP_FUSED_ARGMIN)
        ctx.sweep_refine_depth()
        depth = ctx.sweep_result_pointers()[0]
        argmin, fuse, sweep = (mvs_amd.MVS_K_ARGMIN,), (mvs_amd.MVS_K_FUSE,), (mvs_amd.MVS_K_SWEEP,)
        for radius in (1, 2, 3, 4):
            for tag, tau in (("", 255), ("_gated", TAU)):
                fit = spread(event_ms(ctx, lambda: ctx.depth_fit(depth, radius, tau, step, 6, fetch=False), argmin, iters, warmup))
                mean = spread(event_ms(ctx, lambda: ctx.depth_filter(depth, radius, tau, step, None, False, True, fetch=False), argmin, iters, warmup))
                floor = W * H * (4 + 16 + 1 + (1 if tau < 255 else 0))
                rec["fit_r%d%s" % (radius, tag)] = {"ms": fit, "mean_stage_ms": mean, "over_mean_stage": round(fit["median"] / mean["median"], 3), "bytes_floor": floor,
                                                     "ns_per_pixel": round(fit["median"] * 1e6 / (W * H), 4), "floor_GB_per_s": round(floor / (fit["median"] * 1e6), 1)}
        rec["fit_normals"] = {"ms": spread(event_ms(ctx, lambda: ctx.depth_fit_normals(main_cam, fetch=False), fuse, iters, warmup))}
        maps, plane = ctx.depth_fit_pointers()[0], 4 * W * H

        def seeded():
            ctx.propagate_set_slopes(maps + plane, maps + 2 * plane)
            ctx.propagate_init(depth, mvs_amd.MVS_COST_ZNCC, 2)

        rec["propagate_init"] = {"ms": spread(event_ms(ctx, lambda: ctx.propagate_init(depth, mvs_amd.MVS_COST_ZNCC, 2), sweep, iters, warmup))}
        rec["propagate_init_recorded_slopes"] = {"ms": spread(event_ms(ctx, seeded, sweep, iters, warmup))}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    recs = [one(W, H, a.iters, a.warmup) for W, H in SIZES]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
