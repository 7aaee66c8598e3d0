"""Time the ZNCC sweep (csrc/zncc.hip) against the windowed absolute difference, in one process, after warm-up.

The two cases of tools/time_band.py: 640 x 480 x 32 planes x 4 views on the cameras of the bundled zatisi.yaml (noise frames) and
1920 x 1080 x 32 planes x 16 views of the synthetic scene on ring cameras turned by 0.012 rad (no view rectified).  In each, at radius
1, 2, 3 and 4:
  (a) mvs_sweep_run_zncc(VOLUME | FUSED);
  (b) what a user would otherwise run: mvs_sweep_run(VOLUME | NO_RECT) followed by mvs_sweep_window(radius, 255, NULL, MVS_WINDOW_SELECT).
Both are HIP-event times of the launches (mvs_profile_read: MVS_K_SWEEP for (a), MVS_K_SWEEP + MVS_K_ARGMIN for (b)), one reading per
iteration: the median of --iters iterations with the minimum and maximum beside it, ns per (pixel x plane x view), and the ratio (a) / (b).
One JSON line per case; --out FILE writes the list.

    python tools/time_zncc.py [--iters 20] [--out profiles/zncc/times.json]
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
PLANES = 32


def one(name, W, H, main_cam, main_img, side_cams, sides, iters):
    V = len(sides)
    samples = W * H * PLANES * V
    rec = {"case": name, "size": "%dx%d" % (W, H), "planes": PLANES, "views": V, "iters": iters, "date": datetime.date.today().isoformat()}
    with mvs_amd.Context(W, H) as ctx:
        rec["device"] = ctx.info()
        ctx.sweep_set(main_cam, main_img, side_cams, sides, PLANES)
        for r in (1, 2, 3, 4):
            def windowed():
                ctx.sweep_run(0, V, VOLUME | NO_RECT)
                ctx.sweep_window(r, 255, None, select=True)

            zncc = spread(kernel_ms(ctx, lambda: ctx.sweep_run_zncc(r, 0, V, VOLUME | FUSED), iters))
            sad = spread(kernel_ms(ctx, windowed, iters, (mvs_amd.MVS_K_SWEEP, mvs_amd.MVS_K_ARGMIN)))
            rec["r%d" % r] = {"zncc_ms": zncc, "zncc_ns_per_sample": round(zncc["median"] * 1e6 / samples, 5),
                              "windowed_sad_ms": sad, "windowed_sad_ns_per_sample": round(sad["median"] * 1e6 / samples, 5),
                              "zncc_over_windowed_sad": round(zncc["median"] / sad["median"], 3)}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    recs = [one(*c, a.iters) for c in cases()]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
