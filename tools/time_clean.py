"""Time mvs_sweep_clean (csrc/clean.hip) through mvs_profile_read(MVS_K_ARGMIN): the maps of a 4-view sweep of synth.make_views with
128 planes, at 640 x 480 and 1920 x 1080, each rule alone and all three together (min_views 2, uniqueness 10, speckle 100 / 1), after
warm-up.  The maps are restored before every call (mvs_sweep_argmin, or mvs_sweep_aggregate where rule 2 reads S) with the profile
switched off, so only the cleaning is timed.  Beside the time of every case that runs rule 2: the bytes its pass over the planes must
move (4 per cell of the packed volume, 2 more per cell of S with MVS_CLEAN_SCORES_AGGREGATED) divided by 8 TB/s.
One JSON line per case; --out FILE also writes them as a JSON list.

    python tools/time_clean.py [--iters 10] [--out profiles/clean/times.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mesh-reconstruction_amd", "python"))

import mvs_amd  # noqa: E402
from mvs_amd import synth  # noqa: E402

HBM_TBS = 8.0
PLANES, VIEWS = 128, 4
# name, (min_views, uniqueness, speckle_min_size, speckle_max_diff), aggregated
CASES = (("rule 1", (2, 0, 0, 1), False), ("rule 2", (0, 10, 0, 1), False), ("rule 2 on S", (0, 10, 0, 1), True), ("rule 3", (0, 0, 100, 1), False),
         ("all, winner-take-all", (2, 10, 100, 1), False), ("all, aggregated", (2, 10, 100, 1), True))


def one(W, H, iters):
    main_cam, main_img, side_cams, sides, _ = synth.make_views(W, H, VIEWS, radius=0.3)
    recs = []
    with mvs_amd.Context(W, H) as ctx:
        ctx.sweep_set(main_cam, main_img, side_cams, sides, PLANES)
        ctx.sweep_run(0, VIEWS, mvs_amd.MVS_SWEEP_VOLUME)
        ctx.sweep_aggregate(8)
        for name, params, aggregated in CASES:
            def restore():
                if aggregated:
                    ctx.sweep_aggregate(8)
                else:
                    ctx.sweep_argmin()
            for _ in range(2):
                restore()
                ctx.sweep_clean(*params, aggregated=aggregated)
            ctx.synchronize()
            ctx.profile_read(reset=True)
            for _ in range(iters):
                restore()
                ctx.profile_enable(True)
                ctx.sweep_clean(*params, aggregated=aggregated)
                ctx.profile_enable(False)
            ms, n = ctx.profile_read(reset=True)
            report = ctx.sweep_clean_report()
            t = ms[mvs_amd.MVS_K_ARGMIN] / max(n[mvs_amd.MVS_K_ARGMIN], 1)
            rec = {"size": "%dx%d" % (W, H), "planes": PLANES, "case": name, "min_views": params[0], "uniqueness": params[1], "speckle_min_size": params[2],
                   "speckle_max_diff": params[3], "aggregated": aggregated, "iters": n[mvs_amd.MVS_K_ARGMIN], "clean_ms": round(t, 4), "report": report}
            if params[1]:
                per_cell = 6 if aggregated else 4
                floor_ms = W * H * PLANES * per_cell / (HBM_TBS * 1e12) * 1e3
                rec.update({"bytes_per_cell": per_cell, "bytes_floor_ms_at_8TBs": round(floor_ms, 4), "times_the_floor": round(t / floor_ms, 1)})
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
