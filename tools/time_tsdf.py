"""Time mvs_tsdf_integrate and mvs_tsdf_surface (csrc/tsdf.hip): 16 exact depth maps of synth.Scene (cameras on a ring of radius 0.15) into a
cube over the centre view's frustum, at 640 x 480 and 1920 x 1080, G = 256 and 512.  Integration: mvs_profile_read(MVS_K_TSDF) per call of
16 slots (HIP events around the w-map and integration launches) after warm-up; surface: the wall time of mvs_tsdf_surface (field, mesher,
downloads).  The vector instructions per (node, slot) are counted in the ISA of tsdf_integrate_kernel (hipcc -S, the Makefile's flags): the
unrolled batch of 8 slots is 493 VALU instructions on the full path, 61.6 per (node, slot); the issue share counts only the (node,
slot) pairs that reach the gather (in front of the camera, inside its frame).  One JSON line per case; --out FILE also writes
them as a JSON list.

    python tools/time_tsdf.py [--iters 20] [--out profiles/tsdf/time_tsdf.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mesh-reconstruction_amd", "python"))
import numpy as np  # noqa: E402

import mvs_amd  # noqa: E402
from mvs_amd import synth  # noqa: E402

VALU_PER_NODE_SLOT = 61.6
SIMDS, CLOCK_HZ = 256 * 4, 2.4e9        # MI355X: 256 CUs of 4 SIMDs; a wave64 vector instruction issues over 4 cycles
WAVE_ISSUE_PER_S = SIMDS * CLOCK_HZ / 4.0
HBM_TBS = 8.0
NSLOTS = 16


def in_frame_share(cams, W, H, origin, side, G=64):
    """share of (node, slot) pairs in front of the camera and inside its frame (float64, on a G^3 sample of the cube): only those run the
    whole path; the others leave after the w-row test or the frame test"""
    t = np.linspace(0.0, side, G)
    z, y, x = np.meshgrid(origin[2] + t, origin[1] + t, origin[0] + t, indexing="ij")
    X = np.stack([x.ravel(), y.ravel(), z.ravel(), np.ones(x.size)])
    hit = 0
    for cam in cams:
        q = cam.astype(np.float64) @ X
        with np.errstate(all="ignore"):
            u, v = q[0] / q[3], q[1] / q[3]
        hit += int(((q[3] > 0) & (np.abs(u) <= 1) & (np.abs(v) <= 1)).sum())
    return hit / float(X.shape[1] * len(cams))


def one(W, H, Gs, iters):
    sc = synth.Scene(freq_scale=W / 1920.0)
    cams, depths = [], []
    for a in 2 * np.pi * np.arange(NSLOTS) / NSLOTS:
        c = (0.15 * np.cos(a), 0.15 * np.sin(a), 0.0)
        cams.append(synth.camera_at(c, W, H))
        depths.append(sc.render(c, W, H, want_depth=True)[1])
    recs = []
    with mvs_amd.Context(W, H) as ctx:
        ctx.depth_store(NSLOTS)
        for s in range(NSLOTS):
            ctx.depth_upload(s, cams[s], depths[s])
        half_x = 3.55 / float(cams[0][0, 0])
        side = 2.0 * half_x * 1.01
        origin = np.array([-side / 2, -side / 2, -3.6], np.float32)
        for G in Gs:
            h = np.float32(side / (G - 1))
            ctx.tsdf_volume(G, origin, h, 4 * h)
            for _ in range(3):
                ctx.tsdf_integrate(range(NSLOTS))
            ctx.synchronize()
            ctx.profile_enable(True)
            ctx.profile_read(reset=True)
            for _ in range(iters):
                ctx.tsdf_integrate(range(NSLOTS))
            ms, n = ctx.profile_read(reset=True)
            ctx.profile_enable(False)
            integrate_ms = ms[mvs_amd.MVS_K_TSDF] / max(n[mvs_amd.MVS_K_TSDF], 1)
            # the surface of a fresh volume of the 16 slots (the field above holds 3 + iters passes: the same surface, but time one pass)
            ctx.tsdf_volume(G, origin, h, 4 * h)
            ctx.tsdf_integrate(range(NSLOTS))
            v, f = ctx.tsdf_surface(1)
            walls = []
            for _ in range(max(3, iters // 4)):
                t0 = time.perf_counter()
                s = C.c_void_p()
                ctx._check(ctx.lib.mvs_tsdf_surface(ctx.h, 1, C.byref(s)))
                walls.append((time.perf_counter() - t0) * 1e3)
                ctx.lib.mvs_surface_free(s)
            nodes = G ** 3
            inside = in_frame_share(cams, W, H, origin, side)
            wave_instr = nodes / 64.0 * NSLOTS * inside * VALU_PER_NODE_SLOT   # the (node, slot) pairs that reach the gather
            vol_bytes = 16 * nodes + NSLOTS * W * H * (4 + 4)   # (sum, count) read and written; w-map pass: a depth read and a w write
            rec = {
                "size": "%dx%d" % (W, H), "G": G, "slots": NSLOTS, "iters": iters,
                "integrate_ms": round(integrate_ms, 4),
                "target_ms": {(640, 256): 0.5, (640, 512): 4.0}.get((W, G)),
                "surface_ms_with_downloads": round(float(np.median(walls)), 3),
                "vertices": int(len(v)), "faces": int(len(f)),
                "valu_instr_per_node_slot": VALU_PER_NODE_SLOT,
                "in_frame_share_of_node_slots": round(inside, 4),
                "valu_issue_share_at_integrate_time": round(wave_instr / (integrate_ms * 1e-3) / WAVE_ISSUE_PER_S, 3),
                "hbm_share_at_integrate_time": round(vol_bytes / (integrate_ms * 1e-3) / (HBM_TBS * 1e12), 4),
            }
            print(json.dumps(rec), flush=True)
            recs.append(rec)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    recs = []
    for W, H in ((640, 480), (1920, 1080)):
        recs += one(W, H, (256, 512), a.iters)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
