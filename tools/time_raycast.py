"""Time mvs_tsdf_raycast (csrc/raycast.hip) on tools/time_tsdf.py's volumes: 16 exact depth maps of synth.Scene (cameras on a ring of radius
0.15) into a cube over the centre view's frustum, at 640 x 480 and 1920 x 1080, G = 256 and 512, truncation 4 h, step 0.5; cast from the
centre camera and from one turned by 30 degrees about y.

Per case, in one session: after warm-up of both variants, `--rounds` rounds that alternate the plain march and the march with the brick
mask (the library's test hook mvs_test_raycast_plain), each round `--iters` calls timed by mvs_profile_read(MVS_K_TSDF) (HIP events around
the call's launches; the field and the brick mask are kept between calls, so a steady-state call is the ray kernel alone); the median over
the rounds and their spread (min, max).  `cold_ms`: one call right after the field went stale (field pass + brick pass + ray kernel).
Beside it the mesh route on the same volume: the wall time of mvs_tsdf_surface (mesher, download; its field pass is kept too, which
favours this route), mvs_load_mesh and mvs_depth (which downloads the map), and for a like-for-like figure the wall time of a raycast with
the download of its depth map.  The two variants' maps are compared byte for byte.  One JSON line per case; --out FILE also writes them
as a JSON list.

    python tools/time_raycast.py [--iters 20] [--rounds 5] [--out profiles/raycast/time_raycast.json]
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

NSLOTS = 16
STEP = 0.5


def turned_camera(W, H, deg=30.0):
    """a camera at (1.5, 0, -0.4) turned by `deg` about y: it looks along (-sin, 0, -cos), at the middle of the height field"""
    a = np.radians(deg)
    rot = np.array([[np.cos(a), 0, -np.sin(a)], [0, 1, 0], [np.sin(a), 0, np.cos(a)]])
    return synth.camera_at((1.5, 0.0, -0.4), W, H, rot=rot)


def event_ms(ctx, cam, iters):
    ctx.profile_enable(True)
    ctx.profile_read(reset=True)
    for _ in range(iters):
        ctx.tsdf_raycast(cam, 1, STEP, fetch=False)
    ms, n = ctx.profile_read(reset=True)
    ctx.profile_enable(False)
    return ms[mvs_amd.MVS_K_TSDF] / max(n[mvs_amd.MVS_K_TSDF], 1)


def wall_ms(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), float(min(out)), float(max(out))


def one(W, H, Gs, iters, rounds):
    sc = synth.Scene(freq_scale=W / 1920.0)
    cams, depths = [], []
    for a in 2 * np.pi * np.arange(NSLOTS) / NSLOTS:
        c = (0.15 * np.cos(a), 0.15 * np.sin(a), 0.0)
        cams.append(synth.camera_at(c, W, H))
        depths.append(sc.render(c, W, H, want_depth=True)[1])
    views = {"centre": synth.camera_at((0.0, 0.0, 0.0), W, H), "turned30": turned_camera(W, H)}
    recs = []
    with mvs_amd.Context(W, H) as ctx:
        plain = lambda on: ctx._check(ctx.lib.mvs_test_raycast_plain(ctx.h, int(on)))   # noqa: E731
        ctx.depth_store(NSLOTS)
        for s in range(NSLOTS):
            ctx.depth_upload(s, cams[s], depths[s])
        half_x = 3.55 / float(cams[0][0, 0])
        side = 2.0 * half_x * 1.01
        origin = np.array([-side / 2, -side / 2, -3.6], np.float32)
        for G in Gs:
            h = np.float32(side / (G - 1))
            ctx.tsdf_volume(G, origin, h, 4 * h)
            ctx.tsdf_integrate(range(NSLOTS))
            for name, cam in views.items():
                maps = {}
                for variant in (True, False):          # warm-up, and the two variants' maps
                    plain(variant)
                    for _ in range(3):
                        maps[variant] = ctx.tsdf_raycast(cam, 1, STEP)
                same = maps[True][0].tobytes() == maps[False][0].tobytes() and maps[True][1].tobytes() == maps[False][1].tobytes()
                t = {True: [], False: []}
                for _ in range(rounds):
                    for variant in (True, False):
                        plain(variant)
                        t[variant].append(event_ms(ctx, cam, iters))
                cold = {}
                for variant in (True, False):
                    plain(variant)
                    c = []
                    for _ in range(3):
                        ctx.tsdf_raycast(cam, 2, STEP, fetch=False)   # another min_observations: the field of 1 goes stale
                        c.append(event_ms(ctx, cam, 1))
                    cold[variant] = float(np.median(c))
                plain(False)
                ray_wall = wall_ms(lambda: ctx.tsdf_raycast(cam, 1, STEP), 5)

                def mesh_route():
                    v, f = ctx.tsdf_surface(1)
                    ctx.load_mesh(v, f)
                    return ctx.depth(cam)

                mesh_depth = mesh_route()
                mesh_wall = wall_ms(mesh_route, 5)
                d = maps[False][0]
                both = (d < 1) & (mesh_depth < 1)
                rec = {
                    "size": "%dx%d" % (W, H), "G": G, "camera": name, "step_nodes": STEP, "iters": iters, "rounds": rounds,
                    "hit_share": round(float((d < 1).mean()), 4),
                    "plain_ms": round(float(np.median(t[True])), 4), "plain_ms_min_max": [round(min(t[True]), 4), round(max(t[True]), 4)],
                    "skip_ms": round(float(np.median(t[False])), 4), "skip_ms_min_max": [round(min(t[False]), 4), round(max(t[False]), 4)],
                    "variants_same_bytes": bool(same),
                    "cold_plain_ms": round(cold[True], 4), "cold_skip_ms": round(cold[False], 4),
                    "raycast_wall_ms_with_download": [round(x, 3) for x in ray_wall],
                    "mesh_route_wall_ms": [round(x, 3) for x in mesh_wall],
                    "median_abs_dz_vs_mesh_route": float(np.median(np.abs(d[both] - mesh_depth[both]))) if both.any() else None,
                }
                print(json.dumps(rec), flush=True)
                recs.append(rec)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="640x480,1920x1080")
    ap.add_argument("--grids", default="256,512")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    recs = []
    for size in a.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        recs += one(W, H, [int(g) for g in a.grids.split(",")], a.iters, a.rounds)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
