"""Time mvs_propagate_normals and mvs_fuse_depth_normals (csrc/normals.hip) at 640 x 480 and 1920 x 1080 with K = 4
voters and a normal plane on every slot, beside mvs_fuse_depth_masked on the same inputs in the same process.  Kernel time from
mvs_profile_read(MVS_K_FUSE) (HIP events around the launches of one call), one reading per call after warm-up: median of 20 readings with
min and max.  Nothing is gated.

    python tools/time_fuse_normals.py [--readings 20] [--out profiles/fuse_normals/times.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mesh-reconstruction_amd", "python"))
import numpy as np  # noqa: E402

import mvs_amd  # noqa: E402
from mvs_amd import synth  # noqa: E402

WARMUP = 5


def readings(ctx, call, n):
    for _ in range(WARMUP):
        call()
    ctx.profile_enable(True)
    out = []
    for _ in range(n):
        ctx.profile_read(reset=True)
        call()
        ctx.synchronize()
        ms, launches = ctx.profile_read(reset=True)
        out.append(ms[mvs_amd.MVS_K_FUSE])
    ctx.profile_enable(False)
    return {"median_ms": round(float(np.median(out)), 4), "min_ms": round(float(np.min(out)), 4), "max_ms": round(float(np.max(out)), 4), "readings": n}


def one(W, H, n):
    sc = synth.Scene(freq_scale=W / 1920.0)
    centres = [(0.0, 0.0, 0.0)] + [(0.15 * np.cos(a), 0.15 * np.sin(a), 0.0) for a in 2 * np.pi * np.arange(4) / 4]
    cams = [synth.camera_at(c, W, H) for c in centres]
    views = [sc.render(c, W, H, want_depth=True) for c in centres]
    nb = [1, 2, 3, 4]
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        ctx.depth_store(5)
        for s in range(5):
            ctx.depth_upload(s, cams[s], views[s][1])
            ctx.depth_support_upload(s, np.full((H, W), 3, np.uint8))
        # the hypotheses: each slot's own map with the slopes its neighbours give (mvs_propagate_init with MVS_PROPAGATE_SLOPES, no iteration)
        ctx.sweep_set_main(cams[0], views[0][0])
        ctx.sweep_set_views(np.stack(cams[1:]), [v[0] for v in views[1:]])
        for s in (4, 3, 2, 1, 0):
            ctx.propagate_init(ctx.depth_slot_pointer(s), mvs_amd.MVS_COST_ABSDIFF, 1, 2, slopes=True)
            ctx.depth_normals_upload_device(s, ctx.propagate_normals(cams[s], fetch=False))
        rec = {"size": "%dx%d" % (W, H), "K": 4, "pixels": W * H}
        rec["propagate_normals"] = readings(ctx, lambda: ctx.propagate_normals(cams[0], fetch=False), n)
        kept = {}

        def masked():
            kept["masked"] = len(ctx.fuse_depth(0, nb, copy=False, min_support=2))

        def normals():
            kept["normals"] = len(ctx.fuse_depth(0, nb, copy=False, min_support=2, min_normal_cos=0.9))

        rec["fuse_depth_masked"] = readings(ctx, masked, n)
        rec["fuse_depth_normals"] = readings(ctx, normals, n)
        rec["rows_masked"], rec["rows_normals"] = kept["masked"], kept["normals"]
        rec["normals_over_masked"] = round(rec["fuse_depth_normals"]["median_ms"] / rec["fuse_depth_masked"]["median_ms"], 3)
        # by bytes: both passes read the reference map and its support and gather (depth 4 + support 1) per voter; the normals add 12 per
        # voter read and 12 for the reference
        rec["bytes_per_pixel_masked"] = 2 * (5 + 4 * 5)
        rec["bytes_per_pixel_normals"] = 2 * (5 + 12 + 4 * (5 + 12))
        rec["bytes_ratio"] = round(rec["bytes_per_pixel_normals"] / rec["bytes_per_pixel_masked"], 3)
        return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--readings", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    recs = []
    for W, H in ((640, 480), (1920, 1080)):
        r = one(W, H, a.readings)
        print(json.dumps(r), flush=True)
        recs.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
