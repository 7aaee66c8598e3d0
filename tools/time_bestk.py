"""Time the occlusion-robust sweep (csrc/bestk.hip) against the summing sweeps, in one process, after warm-up.

The two cases of tools/time_band.py: 640 x 480 x 32 planes x 4 views on the cameras of the bundled zatisi.yaml (noise frames) and
1920 x 1080 x 32 planes x 16 views of the synthetic scene on ring cameras turned by 0.012 rad (no view rectified).  In each, at radius 2
with volume and selection:
  (a) mvs_sweep_run_bestk with MVS_COST_ZNCC at keep = 2, 4, 8 and MVS_KEEP_ALL, and mvs_sweep_run_zncc beside them;
  (b) mvs_sweep_run_bestk with MVS_COST_ABSDIFF at the same keeps, and what a user would otherwise run beside them:
      mvs_sweep_run(VOLUME | NO_RECT) followed by mvs_sweep_window(2, 255, NULL, MVS_WINDOW_SELECT).
All are HIP-event times of the launches (mvs_profile_read: MVS_K_SWEEP, for the pair MVS_K_SWEEP + MVS_K_ARGMIN), one reading per
iteration.  The variants are timed in turn, and the whole turn is repeated --passes times, so that a drift of the machine falls on all of
them: the figure is the median of passes x iters readings with the minimum and maximum beside it, ns per (pixel x plane x view), and the
ratio to the summing reference of the same cost.  MVS_KEEP_ALL over mvs_sweep_run_zncc is the skeleton's own overhead (the same cells:
the record says whether the two volumes were equal).  One JSON line per case; --out FILE writes the list.

    python tools/time_bestk.py [--iters 10] [--passes 2] [--out profiles/bestk/times.json]
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
from time_band import cases, kernel_ms, spread  # noqa: E402

VOLUME, FUSED, NO_RECT = mvs_amd.MVS_SWEEP_VOLUME, mvs_amd.MVS_SWEEP_FUSED_ARGMIN, mvs_amd.MVS_SWEEP_NO_RECT
ZNCC, ABSDIFF, KEEP_ALL = mvs_amd.MVS_COST_ZNCC, mvs_amd.MVS_COST_ABSDIFF, mvs_amd.MVS_KEEP_ALL
PLANES, RADIUS, KEEPS = 32, 2, (2, 4, 8, KEEP_ALL)
SWEEP, PAIR = (mvs_amd.MVS_K_SWEEP,), (mvs_amd.MVS_K_SWEEP, mvs_amd.MVS_K_ARGMIN)


def one(name, W, H, main_cam, main_img, side_cams, sides, iters, passes):
    V = len(sides)
    samples = W * H * PLANES * V
    rec = {"case": name, "size": "%dx%d" % (W, H), "planes": PLANES, "views": V, "radius": RADIUS, "iters": iters, "passes": passes,
           "date": datetime.date.today().isoformat()}
    with mvs_amd.Context(W, H) as ctx:
        rec["device"] = ctx.info()
        ctx.sweep_set(main_cam, main_img, side_cams, sides, PLANES)

        def windowed():
            ctx.sweep_run(0, V, VOLUME | NO_RECT)
            ctx.sweep_window(RADIUS, 255, None, select=True)

        def bestk(cost, keep):
            return lambda: ctx.sweep_run_bestk(cost, RADIUS, keep, 0, V, VOLUME | FUSED)

        variants = [("zncc", lambda: ctx.sweep_run_zncc(RADIUS, 0, V, VOLUME | FUSED), SWEEP), ("windowed_sad", windowed, PAIR)]
        for cost, tag in ((ZNCC, "bestk_zncc"), (ABSDIFF, "bestk_absdiff")):
            variants += [("%s_keep_%s" % (tag, keep or "all"), bestk(cost, keep), SWEEP) for keep in KEEPS]
        ms = {key: [] for key, _, _ in variants}
        for _ in range(passes):
            for key, call, kinds in variants:
                ms[key] += kernel_ms(ctx, call, iters, kinds)
        for key in ms:
            s = spread(ms[key])
            base = spread(ms["zncc" if "zncc" in key else "windowed_sad"])["median"]
            rec[key] = {"ms": s, "ns_per_sample": round(s["median"] * 1e6 / samples, 5), "over_summing": round(s["median"] / base, 3)}
        # the same cells: MVS_KEEP_ALL with the ZNCC cost is the ZNCC sweep
        ctx.sweep_run_zncc(RADIUS, 0, V, VOLUME)
        summed = ctx.sweep_fetch(want_volume=True)[3]
        ctx.sweep_run_bestk(ZNCC, RADIUS, KEEP_ALL, 0, V, VOLUME)
        rec["keep_all_equals_zncc"] = bool((ctx.sweep_fetch(want_volume=True)[3] == summed).all())
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
