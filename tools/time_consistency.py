"""Time one propagation iteration with the geometric term (csrc/propagate.hip) on 0, 2, 4 and 8 neighbour slots, in
one process, after warm-up.

The two cases of tools/time_propagate.py (640 x 480 x 4 views on the cameras of the bundled zatisi.yaml, noise frames; 1920 x 1080 x 16
views of the synthetic scene on ring cameras turned by 0.012 rad), its start map (the refined map of a 16-plane mvs_sweep_run_bestk) and
its arguments: ZNCC at radius 2, keep 2, nrandom 2, dz half a coarse step, dg an eighth.  The depth store has eight slots, slot j with
side camera j mod V and the start map as its depth map (what a map holds changes which lanes of a wave answer, not what a lane computes:
the term has no branches).  Per number of slots: mvs_propagate_init with the term recorded (weight 2.5, cap 3 px), then the iterations, as
tools/time_propagate.py times them -- HIP-event times of the launches (mvs_profile_read: MVS_K_SWEEP), one reading per call; the arms
are timed in turn and the turn is repeated --passes times; the figure is the median of passes x iters readings with the minimum and
maximum beside it, and the ratio to the 0-slot arm.

--parent FILE [FILE]: times.json files that tools/time_propagate.py of the PARENT commit wrote in the same session; their
iteration_keep_2 medians are recorded beside the 0-slot arm with the spread of the parent's runs as the margin.

    python tools/time_consistency.py [--iters 10] [--passes 2] [--parent A.json B.json] [--out profiles/consistency/times.json]
"""
import argparse
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mesh-reconstruction_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402  (the HIP runtime first)

import mvs_amd  # noqa: E402
from time_band import cases, kernel_ms, spread  # noqa: E402

BOTH = mvs_amd.MVS_SWEEP_VOLUME | mvs_amd.MVS_SWEEP_FUSED_ARGMIN
ZNCC, KEEP_ALL = mvs_amd.MVS_COST_ZNCC, mvs_amd.MVS_KEEP_ALL
COARSE, RADIUS, KEEP, NRANDOM, WEIGHT, MAX_PX = 16, 2, 2, 2, 2.5, 3.0
SLOTS = (0, 2, 4, 8)


def one(name, W, H, main_cam, main_img, side_cams, sides, iters, passes, parent):
    V = len(sides)
    step = 2.0 / COARSE
    rec = {"case": name, "size": "%dx%d" % (W, H), "views": V, "cost": "zncc", "radius": RADIUS, "keep": KEEP, "nrandom": NRANDOM, "weight": WEIGHT,
           "max_px": MAX_PX, "iters": iters, "passes": passes, "date": datetime.date.today().isoformat()}
    with mvs_amd.Context(W, H) as ctx:
        rec["device"] = ctx.info()
        ctx.sweep_set(main_cam, main_img, side_cams, sides, COARSE)
        ctx.sweep_run_bestk(ZNCC, RADIUS, KEEP_ALL, 0, V, BOTH)
        ctx.sweep_refine_depth()
        start = torch.as_tensor(ctx.depth_device_array(), device="cuda").clone()
        torch.cuda.synchronize()
        ctx.depth_store(8)
        for j in range(8):
            ctx.depth_upload_device(j, side_cams[j % V], start.data_ptr())
        ms = {"init_%d_slots" % n: [] for n in SLOTS}
        ms.update({"iteration_%d_slots" % n: [] for n in SLOTS})
        support = {}
        for _ in range(passes):
            for n in SLOTS:                  # (an arm's iterations follow its own init)
                ctx.propagate_set_consistency(range(n), WEIGHT, MAX_PX)
                ms["init_%d_slots" % n] += kernel_ms(ctx, lambda: ctx.propagate_init(start.data_ptr(), ZNCC, RADIUS, KEEP), iters)
                ms["iteration_%d_slots" % n] += kernel_ms(ctx, lambda: ctx.propagate_run(1, 0.5 * step, 0.125 * step, NRANDOM, 0), iters)
                support[n] = float(ctx.propagate_support().mean())
        ctx.propagate_set_consistency(())
        for key in ms:
            s = spread(ms[key])
            rec[key] = {"ms": s, "over_0_slots": round(s["median"] / spread(ms[key.split("_")[0] + "_0_slots"])["median"], 3)}
        rec["mean_support_after_timing"] = {str(n): round(v, 3) for n, v in support.items()}
    mine = rec["iteration_0_slots"]["ms"]["median"]
    theirs = [r["iteration_keep_2"]["ms"]["median"] for recs in parent for r in recs if r["case"] == name]
    if theirs:
        margin = max(theirs) - min(theirs)
        rec["parent_iteration_keep_2_ms"] = theirs
        rec["parent_spread_ms"] = round(margin, 5)
        rec["iteration_0_slots_over_parent"] = round(mine / (sum(theirs) / len(theirs)), 4)
        rec["within_parent_spread"] = bool(mine <= max(theirs) + margin)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--parent", nargs="*", default=[])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    parent = [json.load(open(p)) for p in a.parent]
    recs = [one(*c, a.iters, a.passes, parent) for c in cases()]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
