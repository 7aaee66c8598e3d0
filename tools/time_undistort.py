"""Time mvs_undistort_device (csrc/lens.hip) through mvs_profile_read(MVS_K_PROJECT): koberec's lens at 640 x 480, 1920 x 1080 and
3840 x 2160, for 1 and for 16 frames per launch, device buffers of uniform noise, after warm-up.  Beside every time the bytes floor of the
call -- one read and one write of every frame, 2 W H bytes per frame -- divided by 8 TB/s.  One JSON line per case; --out FILE also writes
them as a JSON list.

    python tools/time_undistort.py [--iters 20] [--out profiles/undistort/times.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mesh-reconstruction_amd", "python"))

import torch  # noqa: E402  (before the library: it binds to the HIP runtime torch brings along)

import mvs_amd  # noqa: E402
from mvs_amd import tracks  # noqa: E402

HBM_TBS = 8.0


def one(W, H, nframes, iters, lens):
    src = torch.randint(0, 256, (nframes, H, W), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    torch.cuda.synchronize()
    with mvs_amd.Context(W, H) as ctx:
        ctx.set_lens(lens["distortion"], (lens["center_x"] * W / lens["width"], lens["center_y"] * H / lens["height"]))
        for _ in range(3):
            ctx.undistort_device(src.data_ptr(), dst.data_ptr(), nframes)
        ctx.synchronize()
        ctx.profile_enable(True)
        ctx.profile_read(reset=True)
        for _ in range(iters):
            ctx.undistort_device(src.data_ptr(), dst.data_ptr(), nframes)
        ms, n = ctx.profile_read(reset=True)
    t = ms[mvs_amd.MVS_K_PROJECT] / max(n[mvs_amd.MVS_K_PROJECT], 1)
    floor_ms = 2.0 * W * H * nframes / (HBM_TBS * 1e12) * 1e3
    return {"size": "%dx%d" % (W, H), "frames": nframes, "iters": n[mvs_amd.MVS_K_PROJECT], "undistort_ms": round(t, 4), "ms_per_frame": round(t / nframes, 5),
            "bytes_floor_ms_at_8TBs": round(floor_ms, 5), "times_the_floor": round(t / floor_ms, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lens = tracks.load("koberec.yaml")
    recs = []
    for W, H in ((640, 480), (1920, 1080), (3840, 2160)):
        for nframes in (1, 16):
            rec = one(W, H, nframes, a.iters, lens)
            print(json.dumps(rec), flush=True)
            recs.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
