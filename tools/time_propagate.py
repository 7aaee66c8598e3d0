"""Time the hypothesis propagation (csrc/propagate.hip) beside the occlusion-robust sweep over 48 planes, in one
process, after warm-up.

The two cases of tools/time_band.py: 640 x 480 x 4 views on the cameras of the bundled zatisi.yaml (noise frames) and 1920 x 1080 x 16
views of the synthetic scene on ring cameras turned by 0.012 rad.  The start map is the refined map of a 16-plane mvs_sweep_run_bestk.
In each, ZNCC at radius 2 with MVS_KEEP_ALL and with keep 2:
  (a) mvs_propagate_init on the start map (the seed kernel and one evaluation of every pixel),
  (b) one iteration, mvs_propagate_run(1, dz = half a coarse step, dg = an eighth, nrandom = 2): two half-passes of up to 10 hypotheses
      per active pixel.  The iterations follow one init, so the hypotheses settle while they are timed,
  (c) mvs_sweep_run_bestk over 48 planes with the same cost, radius and keep, volume and selection.
All are HIP-event times of the launches (mvs_profile_read: MVS_K_SWEEP), one reading per call.  The variants are timed in turn and the
whole turn is repeated --passes times; the figure is the median of passes x iters readings with the minimum and maximum beside it, and
for (a) and (b) the ratio to (c).  There is no gate.  One JSON line per case; --out FILE writes the list.

    python tools/time_propagate.py [--iters 10] [--passes 2] [--out profiles/propagate/times.json]
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
COARSE, PLANES, RADIUS, NRANDOM = 16, 48, 2, 2


def one(name, W, H, main_cam, main_img, side_cams, sides, iters, passes):
    V = len(sides)
    step = 2.0 / COARSE
    rec = {"case": name, "size": "%dx%d" % (W, H), "views": V, "cost": "zncc", "radius": RADIUS, "nrandom": NRANDOM, "sweep_planes": PLANES, "iters": iters,
           "passes": passes, "date": datetime.date.today().isoformat()}
    with mvs_amd.Context(W, H) as ctx:
        rec["device"] = ctx.info()
        ctx.sweep_set(main_cam, main_img, side_cams, sides, COARSE)
        ctx.sweep_run_bestk(ZNCC, RADIUS, KEEP_ALL, 0, V, BOTH)
        ctx.sweep_refine_depth()
        start = torch.as_tensor(ctx.depth_device_array(), device="cuda").clone()
        torch.cuda.synchronize()
        ctx.sweep_set_planes(PLANES, -1.0, 1.0)
        variants = []
        for keep in (KEEP_ALL, 2):
            tag = "keep_%s" % (keep or "all")
            variants += [("init_" + tag, lambda keep=keep: ctx.propagate_init(start.data_ptr(), ZNCC, RADIUS, keep)),
                         ("iteration_" + tag, lambda: ctx.propagate_run(1, 0.5 * step, 0.125 * step, NRANDOM, 0)),
                         ("bestk_48_planes_" + tag, lambda keep=keep: ctx.sweep_run_bestk(ZNCC, RADIUS, keep, 0, V, BOTH))]
        ms = {key: [] for key, _ in variants}
        for _ in range(passes):
            for key, call in variants:       # (an arm's iterations follow its own init)
                ms[key] += kernel_ms(ctx, call, iters)
        for key in ms:
            s = spread(ms[key])
            rec[key] = {"ms": s}
            if not key.startswith("bestk_"):
                rec[key]["over_bestk_48_planes"] = round(s["median"] / spread(ms["bestk_48_planes_" + key.split("_", 1)[1]])["median"], 3)
        rec["report_after_timing"] = ctx.propagate_report()
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    recs = [one(*c, a.iters, a.passes) for c in cases()]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
