"""Time the resolution pyramid (csrc/pyramid.hip) against the sequences it competes with, in one process, after
warm-up.

Two cases: 640 x 480 x 4 views (the synthetic scene on ring cameras) and 1920 x 1080 x 16 general views (ring cameras turned by 0.012 rad:
no view rectified).  In each, four sequences on the same staged frames:
  (a) a 128-plane mvs_sweep_run + mvs_sweep_refine_depth;
  (b) mvs_amd.coarse_to_fine, 16 + 32 planes at one resolution;
  (c) mvs_amd.pyramid_coarse_to_fine on two levels (full, 1/2), 16 + 32 planes;
  (d) the same on three levels (full, 1/2, 1/4), 16 + 32 + 32 planes.
Every sequence is given twice: as a host clock around calls that end in a synchronise of every context involved (it spans the plane-table
uploads, which synchronise, the stage's staging and planning; no map is downloaded), and as HIP-event times of the timed launches per
class (mvs_profile_read of every context, summed over the contexts: MVS_K_SWEEP, MVS_K_ARGMIN, MVS_K_PLAN, MVS_K_PROJECT;
mvs_sweep_refine_depth is not timed by the library).  The frames of the turned ring are those of the unturned cameras, so its depths mean
nothing: it times the kernels on realistic texture, nothing else.  Every figure is the median of --iters iterations with the minimum and
maximum beside it.  One JSON line per case; --out FILE writes the list.

    python tools/time_pyramid.py [--iters 20] [--out profiles/pyramid/times.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mesh-reconstruction_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402,F401
import torch  # noqa: E402,F401  (the HIP runtime first)

import mvs_amd  # noqa: E402
from mvs_amd import synth  # noqa: E402
from time_band import rotated_ring, spread  # noqa: E402

BOTH = mvs_amd.MVS_SWEEP_VOLUME | mvs_amd.MVS_SWEEP_FUSED_ARGMIN
COARSE, BAND, DENSE, STEPS = 16, 32, 128, 1.5
CLASSES = (("sweep", mvs_amd.MVS_K_SWEEP), ("argmin", mvs_amd.MVS_K_ARGMIN), ("plan", mvs_amd.MVS_K_PLAN), ("project", mvs_amd.MVS_K_PROJECT))


def measure(ctxs, call, iters):
    """-> {"wall_ms": spread, "<class>_ms": spread ..., "launch_ms": spread of the classes' sum}"""
    def wait():
        for ctx in ctxs:
            ctx.synchronize()

    for _ in range(3):
        call()
    wait()
    wall = []
    for _ in range(iters):
        t0 = time.perf_counter()
        call()
        wait()
        wall.append((time.perf_counter() - t0) * 1e3)
    for ctx in ctxs:
        ctx.profile_enable(True)
        ctx.profile_read(reset=True)
    per_class = {name: [] for name, _ in CLASSES}
    total = []
    for _ in range(iters):
        call()
        sums = dict.fromkeys(per_class, 0.0)
        for ctx in ctxs:
            ms, _ = ctx.profile_read(reset=True)
            for name, kind in CLASSES:
                sums[name] += float(ms[kind])
        for name in per_class:
            per_class[name].append(sums[name])
        total.append(sum(sums.values()))
    for ctx in ctxs:
        ctx.profile_enable(False)
    rec = {"wall_ms": spread(wall), "launch_ms": spread(total)}
    for name in per_class:
        rec[name + "_ms"] = spread(per_class[name])
    return rec


def cases():
    W, H, V = 640, 480, 4
    yield ("synthetic scene, ring",) + (W, H) + synth.make_views(W, H, V)[:4]
    W, H, V = 1920, 1080, 16
    main_cam, main_img, _, sides, _ = synth.make_views(W, H, V)
    yield "synthetic scene, rotated ring", W, H, main_cam, main_img, rotated_ring(W, H, V), sides


def one(name, W, H, main_cam, main_img, side_cams, sides, iters):
    V = len(sides)
    rec = {"case": name, "size": "%dx%d" % (W, H), "views": V, "planes": {"dense": DENSE, "coarse": COARSE, "band": BAND}, "iters": iters}
    ctxs = [mvs_amd.Context(W >> k, H >> k) for k in range(3)]
    try:
        full = ctxs[0]
        rec["device"] = full.info()
        full.sweep_set(main_cam, main_img, side_cams, sides, COARSE)

        def dense():
            full.sweep_set_planes(DENSE)
            full.sweep_run(0, V, BOTH)
            full.sweep_refine_depth()

        rec["a_dense_%d" % DENSE] = measure(ctxs[:1], dense, iters)
        rec["b_coarse_to_fine"] = measure(ctxs[:1], lambda: mvs_amd.coarse_to_fine(full, COARSE, BAND, STEPS, fetch=False), iters)
        rec["c_pyramid_2_levels"] = measure(ctxs[:2], lambda: mvs_amd.pyramid_coarse_to_fine(ctxs[:2], COARSE, BAND, STEPS, fetch=False), iters)
        rec["d_pyramid_3_levels"] = measure(ctxs, lambda: mvs_amd.pyramid_coarse_to_fine(ctxs, COARSE, BAND, STEPS, fetch=False), iters)
        for key in ("c_pyramid_2_levels", "d_pyramid_3_levels"):
            for other in ("a_dense_%d" % DENSE, "b_coarse_to_fine"):
                for what in ("wall_ms", "launch_ms"):
                    rec["%s_over_%s_%s" % (key[:1], other[:1], what[:-3])] = round(rec[key][what]["median"] / rec[other][what]["median"], 3)
    finally:
        for ctx in ctxs:
            ctx.close()
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
