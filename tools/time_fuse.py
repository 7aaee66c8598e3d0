"""Time mvs_fuse_depth (csrc/fuse.hip) at 640 x 480 and 1920 x 1080 with K = 4 neighbours: kernel time from mvs_profile_read(MVS_K_FUSE)
(HIP events around the count pass, the scan and the row pass) after warm-up, the download of the rows separately, points kept, and the
bytes and vector instructions per pixel from the shapes.  One JSON line per size; --out FILE also writes them as a JSON list.

    python tools/time_fuse.py [--iters 50] [--out profiles/fuse/time_fuse.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mesh-reconstruction_amd", "python"))
import numpy as np  # noqa: E402

import mvs_amd  # noqa: E402
from mvs_amd import synth  # noqa: E402

HBM_TBS = 8.0          # MI355X HBM3E peak, TB/s
VALU_LANE_OPS = 78.6e12  # MI355X FP32 vector peak 157.3 TFLOPS counted as FMAs: vector instructions x lanes per second
# vector instructions per pixel, estimated from the kernel source (a correctly rounded f32 division is about 10 instructions): about 110 for
# the reference back-projection and normal, about 120 per neighbour vote (two projections, a back-projection, seven divisions); the count
# pass and the row pass both do all of it
VALU_PER_PIXEL = lambda K: 2 * (110 + 120 * K)   # noqa: E731


def one(W, H, iters):
    sc = synth.Scene(freq_scale=W / 1920.0)
    centres = [(0.0, 0.0, 0.0)] + [(0.15 * np.cos(a), 0.15 * np.sin(a), 0.0) for a in 2 * np.pi * np.arange(4) / 4]
    with mvs_amd.Context(W, H) as ctx:
        ctx.depth_store(5)
        for s, c in enumerate(centres):
            ctx.depth_upload(s, synth.camera_at(c, W, H), sc.render(c, W, H, want_depth=True)[1])
        nb = [1, 2, 3, 4]
        for _ in range(5):
            rows = ctx.fuse_depth(0, nb, copy=False)
        ctx.profile_enable(True)
        ctx.profile_read(reset=True)
        for _ in range(iters):
            ctx.fuse_depth(0, nb, copy=False)
        ms, n = ctx.profile_read(reset=True)
        kernel_ms = ms[mvs_amd.MVS_K_FUSE] / max(n[mvs_amd.MVS_K_FUSE], 1)
        ctx.profile_enable(False)
        # download: the same call with and without the row copy (the count read-back and synchronisation are in both)
        walls = {True: [], False: []}
        lib, h = ctx.lib, ctx.h
        out = np.zeros((W * H, 7), np.float32)
        ns = np.asarray(nb, np.int32)
        cnt = mvs_amd.C.c_int(0)
        for _ in range(iters):
            for with_rows in (False, True):
                t0 = time.perf_counter()
                lib.mvs_fuse_depth(h, 0, 4, ns.ctypes.data_as(mvs_amd._i32p), 2, 1.0, 0.01, float("inf"),
                                   out.ctypes.data_as(mvs_amd._fp) if with_rows else None, mvs_amd.C.byref(cnt))
                walls[with_rows].append((time.perf_counter() - t0) * 1e3)
        kept = len(rows)
        P = W * H
        read_bytes = 2 * P * 4 * (1 + 4)   # both passes read the reference map and gather one depth per neighbour and pixel
        write_bytes = kept * 28
        valu = VALU_PER_PIXEL(4) * P
        rec = {
            "size": "%dx%d" % (W, H), "K": 4, "iters": iters,
            "kernel_ms": round(kernel_ms, 4),
            "download_ms": round(float(np.median(walls[True]) - np.median(walls[False])), 4),
            "wall_ms_without_rows": round(float(np.median(walls[False])), 4),
            "wall_ms_with_rows": round(float(np.median(walls[True])), 4),
            "points_kept": kept, "pixels": P,
            "bytes_per_pixel": round((read_bytes + write_bytes) / P, 2),
            "valu_instr_per_pixel": VALU_PER_PIXEL(4),
            "hbm_share_of_peak_at_kernel_time": round((read_bytes + write_bytes) / (kernel_ms * 1e-3) / (HBM_TBS * 1e12), 4),
            "valu_share_of_peak_at_kernel_time": round(valu / (kernel_ms * 1e-3) / VALU_LANE_OPS, 4),
            "target_ms": 0.04 if W == 640 else 0.15,
        }
        return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    recs = []
    for W, H in ((640, 480), (1920, 1080)):
        r = one(W, H, a.iters)
        print(json.dumps(r), flush=True)
        recs.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
