"""Time the band sweep with windowed costs (csrc/bestk.hip) beside the sweeps it joins, in one process, after
warm-up.

The two cases of tools/time_band.py: 640 x 480 x 32 planes x 4 views on the cameras of the bundled zatisi.yaml (noise frames) and
1920 x 1080 x 32 planes x 16 views of the synthetic scene on ring cameras turned by 0.012 rad (no view rectified).  The prior is the
refined map of a 16-plane sweep, the 32 offsets span +- 1.5 of its steps.  In each, at radius 2 with volume and selection, four arms --
MVS_COST_ZNCC and MVS_COST_ABSDIFF, each at MVS_KEEP_ALL and keep 2 -- of
  (a) mvs_sweep_run_band_bestk,
  (b) mvs_sweep_run_bestk with the same arguments on the same plane table (the same arithmetic but for one add and a range test per
      sample and the prior of every sample position held in a register),
and beside them (c) what a user has today: mvs_sweep_run_band followed by mvs_sweep_window(2, 255, NULL, MVS_WINDOW_SELECT).
All are HIP-event times of the launches (mvs_profile_read: MVS_K_SWEEP, for (c) MVS_K_SWEEP + MVS_K_ARGMIN), one reading per iteration.
The variants are timed in turn, and the whole turn is repeated --passes times, so that a drift of the machine falls on all of them: the
figure is the median of passes x iters readings with the minimum and maximum beside it, ns per (pixel x plane x view), and for (a) the
ratios to (b) and to (c).  There is no gate.  The record also says whether identity (b) of section 24 held at this size: the absolute
difference at radius 0 with MVS_KEEP_ALL against mvs_sweep_run_band.  One JSON line per case; --out FILE writes the list.

    python tools/time_band_bestk.py [--iters 10] [--passes 2] [--out profiles/band_bestk/times.json]
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

VOLUME, FUSED = mvs_amd.MVS_SWEEP_VOLUME, mvs_amd.MVS_SWEEP_FUSED_ARGMIN
BOTH = VOLUME | FUSED
ZNCC, ABSDIFF, KEEP_ALL = mvs_amd.MVS_COST_ZNCC, mvs_amd.MVS_COST_ABSDIFF, mvs_amd.MVS_KEEP_ALL
COARSE, PLANES, STEPS, RADIUS = 16, 32, 1.5, 2
ARMS = [("zncc", ZNCC, KEEP_ALL), ("zncc", ZNCC, 2), ("absdiff", ABSDIFF, KEEP_ALL), ("absdiff", ABSDIFF, 2)]
SWEEP, PAIR = (mvs_amd.MVS_K_SWEEP,), (mvs_amd.MVS_K_SWEEP, mvs_amd.MVS_K_ARGMIN)


def one(name, W, H, main_cam, main_img, side_cams, sides, iters, passes):
    V = len(sides)
    samples = W * H * PLANES * V
    hb = STEPS * 2.0 / COARSE
    rec = {"case": name, "size": "%dx%d" % (W, H), "planes": PLANES, "views": V, "radius": RADIUS, "iters": iters, "passes": passes,
           "date": datetime.date.today().isoformat()}
    with mvs_amd.Context(W, H) as ctx:
        rec["device"] = ctx.info()
        ctx.sweep_set(main_cam, main_img, side_cams, sides, COARSE)
        ctx.sweep_run(0, V, BOTH)
        ctx.sweep_refine_depth()
        prior = torch.as_tensor(ctx.depth_device_array(), device="cuda").clone()
        torch.cuda.synchronize()
        ctx.sweep_set_planes(PLANES, -hb, hb)

        def band_window():
            ctx.sweep_run_band(prior.data_ptr(), 0, V, VOLUME)
            ctx.sweep_window(RADIUS, 255, None, select=True)

        def band(cost, keep):
            return lambda: ctx.sweep_run_band_bestk(prior.data_ptr(), cost, RADIUS, keep, 0, V, BOTH)

        def table(cost, keep):
            return lambda: ctx.sweep_run_bestk(cost, RADIUS, keep, 0, V, BOTH)

        variants = [("band_then_window", band_window, PAIR)]
        for tag, cost, keep in ARMS:
            variants += [("band_bestk_%s_keep_%s" % (tag, keep or "all"), band(cost, keep), SWEEP), ("bestk_%s_keep_%s" % (tag, keep or "all"), table(cost, keep), SWEEP)]
        ms = {key: [] for key, _, _ in variants}
        for _ in range(passes):
            for key, call, kinds in variants:
                ms[key] += kernel_ms(ctx, call, iters, kinds)
        pair = spread(ms["band_then_window"])["median"]
        for key in ms:
            s = spread(ms[key])
            rec[key] = {"ms": s, "ns_per_sample": round(s["median"] * 1e6 / samples, 5)}
            if key.startswith("band_bestk_"):
                rec[key]["over_bestk"] = round(s["median"] / spread(ms[key[len("band_"):]])["median"], 3)
                rec[key]["over_band_then_window"] = round(s["median"] / pair, 3)
        # the same cells: the absolute difference at radius 0 with MVS_KEEP_ALL is the band sweep
        ctx.sweep_run_band(prior.data_ptr(), 0, V, VOLUME)
        summed = ctx.sweep_fetch(want_volume=True)[3]
        ctx.sweep_run_band_bestk(prior.data_ptr(), ABSDIFF, 0, KEEP_ALL, 0, V, VOLUME)
        rec["radius_0_keep_all_equals_band"] = bool((ctx.sweep_fetch(want_volume=True)[3] == summed).all())
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
