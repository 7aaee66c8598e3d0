"""Time mvs_tsdf_integrate_frames against mvs_tsdf_integrate, and mvs_tsdf_shade (csrc/tsdf.hip, csrc/appearance.hip), on
tools/time_tsdf.py's volumes: 16 exact depth maps of synth.Scene with their frames (cameras on a ring of radius 0.15) into a cube over the
centre view's frustum, at 640 x 480 and 1920 x 1080, G = 256 and 512.  The two integrations alternate in one session, `rounds` times `iters`
calls each after warm-up, mvs_profile_read(MVS_K_TSDF) per call of 16 slots (HIP events around the w-map pass and the integration launch);
the ratio is the yardstick: frames / plain, per round and over all.  Then the centre camera's ray-cast of a fresh volume of the 16 pairs is
shaded `iters` times (events around the one launch).  One JSON line per case; --out FILE also writes them as a JSON list.

    python tools/time_tsdf_appearance.py [--iters 10] [--rounds 3] [--out profiles/tsdf/appearance_times.json]
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

NSLOTS = 16
K = mvs_amd.MVS_K_TSDF


def _timed(ctx, call, iters):
    ctx.synchronize()
    ctx.profile_enable(True)
    ctx.profile_read(reset=True)
    for _ in range(iters):
        call()
    ms, n = ctx.profile_read(reset=True)
    ctx.profile_enable(False)
    return ms[K] / max(n[K], 1)


def one(W, H, Gs, iters, rounds):
    sc = synth.Scene(freq_scale=W / 1920.0)
    cams, depths, frames = [], [], []
    for a in 2 * np.pi * np.arange(NSLOTS) / NSLOTS:
        c = (0.15 * np.cos(a), 0.15 * np.sin(a), 0.0)
        img, d = sc.render(c, W, H, want_depth=True)
        cams.append(synth.camera_at(c, W, H))
        depths.append(d)
        frames.append(img)
    centre = synth.camera_at((0.0, 0.0, 0.0), W, H)
    slots = list(range(NSLOTS))
    recs = []
    with mvs_amd.Context(W, H) as ctx:
        ctx.depth_store(NSLOTS)
        ctx.frame_store(NSLOTS)
        for s in slots:
            ctx.depth_upload(s, cams[s], depths[s])
            ctx.frame_upload(s, frames[s])
        half_x = 3.55 / float(cams[0][0, 0])
        side = 2.0 * half_x * 1.01
        origin = np.array([-side / 2, -side / 2, -3.6], np.float32)
        for G in Gs:
            h = np.float32(side / (G - 1))
            ctx.tsdf_volume(G, origin, h, 4 * h)
            plain = lambda: ctx.tsdf_integrate(slots)                    # noqa: E731
            with_frames = lambda: ctx.tsdf_integrate_frames(slots, slots)   # noqa: E731
            for _ in range(3):
                plain()
                with_frames()
            per_round = []
            for _ in range(rounds):
                per_round.append((_timed(ctx, plain, iters), _timed(ctx, with_frames, iters)))
            plain_ms = float(np.mean([p for p, _ in per_round]))
            frames_ms = float(np.mean([f for _, f in per_round]))
            # the model image: a fresh volume of the 16 pairs, the centre camera's ray-cast, shaded
            ctx.tsdf_volume(G, origin, h, 4 * h)
            with_frames()
            depth, _ = ctx.tsdf_raycast(centre, 1, 0.5)
            dptr = ctx.tsdf_raycast_pointers()[0]
            shaded = ctx.tsdf_shade(centre, dptr)
            shade_ms = _timed(ctx, lambda: ctx.tsdf_shade(centre, dptr, fetch=False), iters)
            nodes = G ** 3
            rec = {
                "size": "%dx%d" % (W, H), "G": G, "pairs": NSLOTS, "iters": iters, "rounds": rounds,
                "integrate_ms": round(plain_ms, 4),
                "integrate_frames_ms": round(frames_ms, 4),
                "ratio": round(frames_ms / plain_ms, 3),
                "ratio_per_round": [round(f / p, 3) for p, f in per_round],
                "shade_ms": round(shade_ms, 4),
                "hit_pixels": int((depth < 1).sum()), "shaded_pixels": int((shaded[..., 1] == 255).sum()),
                # (sum, count) and the cell read and written; the w-map pass: a depth and a frame read, an 8-byte record written
                "bytes_moved_frames": 24 * nodes + NSLOTS * W * H * (4 + 1 + 8),
                "bytes_moved_plain": 16 * nodes + NSLOTS * W * H * (4 + 4),
            }
            print(json.dumps(rec), flush=True)
            recs.append(rec)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    recs = []
    for W, H in ((640, 480), (1920, 1080)):
        recs += one(W, H, (256, 512), a.iters, a.rounds)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
