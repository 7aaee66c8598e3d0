#!/usr/bin/env python3
"""Full-frame sweep times of the three kernel variants (volume + fused depth selection, fused only, volume only) on the bench's ring at
one or more configs: one JSON line per config.  For A/B timings of two builds in one GPU session: MVS_HIP_LIBRARY=<variant> python
tools/time_rect_variants.py c2 c3 (tools/build_variant.sh builds the variant)."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mesh-reconstruction_amd", "python"))
import mvs_amd
from mvs_amd import synth

CONFIGS = {"c1": (640, 480, 32, 4), "c2": (1280, 720, 64, 8), "c3": (1920, 1080, 128, 16), "c3v4": (1920, 1080, 128, 4)}


def t(ctx, V, flags, n=100):
    for _ in range(20):
        ctx.sweep_run(0, V, flags)
    ctx.synchronize()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(n):
            ctx.sweep_run(0, V, flags)
        ctx.synchronize()
        ts.append((time.perf_counter() - t0) / n * 1e3)
    return ts


for name in sys.argv[1:] or ["c3"]:
    W, H, D, V = CONFIGS[name]
    main_cam, main_img, side_cams, sides, _ = synth.make_views(W, H, V, radius=0.15)
    with mvs_amd.Context(W, H) as ctx:
        ctx.sweep_set(main_cam, main_img, side_cams, sides, D)
        res = {"both": t(ctx, V, mvs_amd.MVS_SWEEP_VOLUME | mvs_amd.MVS_SWEEP_FUSED_ARGMIN), "fused_only": t(ctx, V, mvs_amd.MVS_SWEEP_FUSED_ARGMIN),
               "volume_only": t(ctx, V, mvs_amd.MVS_SWEEP_VOLUME)}
        shape = ctx.plan_shape()
    print(json.dumps({"config": name, "library": os.environ.get("MVS_HIP_LIBRARY", "default"), "plan_shape": shape, "ms_three_runs_of_100": res}))
