"""Time the band sweep (csrc/band.hip) against the ordinary sweep's general kernels, in one process, after warm-up.

Two cases: 640 x 480 x 32 planes x 4 views on the cameras of the bundled zatisi.yaml (noise frames, as tools/tracks_sweep_probe.py: the
cameras are what matters to the kernels, and a prior made from noise is the worst case for the band kernel's gathers), and
1920 x 1080 x 32 planes x 16 views of the synthetic scene on ring cameras turned by 0.012 rad (no view rectified).  In each:
  (a) mvs_sweep_run_band(VOLUME | FUSED) with +-1.5 coarse steps around the refined 16-plane sweep;
  (b) mvs_sweep_run(VOLUME | FUSED) on the same plane count, views and flags with MVS_SWEEP_NO_RECT (sweep_fx_tiled) and with
      MVS_SWEEP_FORCE_GENERIC (sweep_fx_generic, the un-tiled kernel whose arithmetic the band kernel shares);
  (c) the whole coarse-to-fine sequence (mvs_amd.coarse_to_fine: 16 + 32 planes, refined twice, resolved) against a 128-plane
      mvs_sweep_run + mvs_sweep_refine_depth.
(a) and (b) are HIP-event times of the launches (mvs_profile_read, MVS_K_SWEEP), one reading per iteration; (c) is given twice: as a host
clock around calls that end in a synchronise (it spans the plane-table uploads, which synchronise, and planning; no map is downloaded on
either side), and as the sum of the HIP-event times of its timed launches.  The ring case's frames are those of the unturned cameras, so
its depths mean nothing (the report's band-edge count shows it): it times the kernels on realistic texture, nothing else.  Every figure
is the median of --iters iterations with the minimum and maximum beside it, and ns per (pixel x plane x view) for the kernels.  One JSON
line per case; --out FILE writes the list.

    python tools/time_band.py [--iters 20] [--out profiles/band/times.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mesh-reconstruction_amd", "python"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (the HIP runtime first)

import mvs_amd  # noqa: E402
from mvs_amd import synth, tracks  # noqa: E402

BOTH = mvs_amd.MVS_SWEEP_VOLUME | mvs_amd.MVS_SWEEP_FUSED_ARGMIN
COARSE, BAND, DENSE, STEPS = 16, 32, 128, 1.5


def spread(values):
    v = sorted(values)
    return {"median": round(v[len(v) // 2], 5), "min": round(v[0], 5), "max": round(v[-1], 5)}


def kernel_ms(ctx, call, iters, kinds=(mvs_amd.MVS_K_SWEEP,)):
    """HIP-event time of the launches of one call that the library times under `kinds`, per iteration"""
    for _ in range(3):
        call()
    ctx.synchronize()
    ctx.profile_enable(True)
    ctx.profile_read(reset=True)
    out = []
    for _ in range(iters):
        call()
        ms, _ = ctx.profile_read(reset=True)
        out.append(float(sum(ms[k] for k in kinds)))
    ctx.profile_enable(False)
    return out


def launch_ms(ctx, call, iters):
    """HIP-event time of every timed launch of one call (sweep, selection and resolve, planning; mvs_sweep_refine_depth is not timed by
    the library), per iteration"""
    return kernel_ms(ctx, call, iters, (mvs_amd.MVS_K_SWEEP, mvs_amd.MVS_K_ARGMIN, mvs_amd.MVS_K_PLAN))


def wall_ms(ctx, call, iters):
    for _ in range(3):
        call()
    ctx.synchronize()
    out = []
    for _ in range(iters):
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def rotated_ring(W, H, V, radius=0.15):
    cams = []
    for v in range(V):
        a = 2.0 * np.pi * v / V
        yaw, pitch = 0.012 * np.cos(a), 0.012 * np.sin(a)
        cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
        rot = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        cams.append(synth.camera_at([radius * np.cos(a), radius * np.sin(a), 0.0], W, H, rot=rot))
    return np.stack(cams)


def cases():
    t = tracks.load("zatisi.yaml")
    W, H, cams = t["width"], t["height"], t["cameras"]
    n = len(cams)
    m, s = n // 2, max(1, n // 12)
    rng = np.random.default_rng(2)
    imgs = [rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(5)]
    yield "zatisi cameras, noise frames", W, H, cams[m], imgs[0], np.stack([cams[i] for i in (m - 2 * s, m - s, m + s, m + 2 * s)]), imgs[1:]
    W, H, V = 1920, 1080, 16
    main_cam, main_img, _, sides, _ = synth.make_views(W, H, V)
    yield "synthetic scene, rotated ring", W, H, main_cam, main_img, rotated_ring(W, H, V), sides


def one(name, W, H, main_cam, main_img, side_cams, sides, iters):
    V = len(sides)
    samples = W * H * BAND * V
    rec = {"case": name, "size": "%dx%d" % (W, H), "planes": BAND, "views": V, "iters": iters}
    hb = STEPS * 2.0 / COARSE
    with mvs_amd.Context(W, H) as ctx:
        rec["device"] = ctx.info()
        ctx.sweep_set(main_cam, main_img, side_cams, sides, COARSE)
        ctx.sweep_run(0, V, BOTH)
        ctx.sweep_refine_depth()
        prior = torch.as_tensor(ctx.depth_device_array(), device="cuda").clone()
        torch.cuda.synchronize()
        ctx.sweep_set_planes(BAND, -hb, hb)
        band = kernel_ms(ctx, lambda: ctx.sweep_run_band(prior.data_ptr(), 0, V, BOTH), iters)
        ctx.sweep_band_resolve(fetch=False)
        rec["band_report"] = ctx.sweep_band_report()
        tiled = kernel_ms(ctx, lambda: ctx.sweep_run(0, V, BOTH | mvs_amd.MVS_SWEEP_NO_RECT), iters)
        rec["plan_shape"] = ctx.plan_shape()
        untiled = kernel_ms(ctx, lambda: ctx.sweep_run(0, V, BOTH | mvs_amd.MVS_SWEEP_FORCE_GENERIC), iters)
        for key, ms in (("band", band), ("tiled_no_rect", tiled), ("untiled_force_generic", untiled)):
            rec[key + "_ms"] = spread(ms)
            rec[key + "_ns_per_sample"] = round(spread(ms)["median"] * 1e6 / samples, 5)
        rec["band_over_untiled"] = round(rec["band_ms"]["median"] / rec["untiled_force_generic_ms"]["median"], 3)
        rec["band_over_tiled"] = round(rec["band_ms"]["median"] / rec["tiled_no_rect_ms"]["median"], 3)

        def two_levels():
            mvs_amd.coarse_to_fine(ctx, COARSE, BAND, STEPS, fetch=False)

        def dense():
            ctx.sweep_set_planes(DENSE)     # (the two-level sequence stages its plane tables too)
            ctx.sweep_run(0, V, BOTH)
            ctx.sweep_refine_depth()

        for key, call in (("coarse_to_fine", two_levels), ("dense_%d" % DENSE, dense)):
            rec[key + "_wall_ms"] = spread(wall_ms(ctx, call, iters))
            rec[key + "_launch_ms"] = spread(launch_ms(ctx, call, iters))
        rec["dense_over_coarse_to_fine_wall"] = round(rec["dense_%d_wall_ms" % DENSE]["median"] / rec["coarse_to_fine_wall_ms"]["median"], 3)
        rec["dense_over_coarse_to_fine_launches"] = round(rec["dense_%d_launch_ms" % DENSE]["median"] / rec["coarse_to_fine_launch_ms"]["median"], 3)
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
