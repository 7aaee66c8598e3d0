"""Time mvs_fuse_sequence (csrc/fuse_sequence.hip) beside the calls it replaces, in one session: 16 references x 4
neighbours (a ring of 16 cameras around synth.Scene, exact maps; every reference's neighbours are the two cameras either side of it) at
640 x 480 and 1920 x 1080.  Per size, alternating within every repetition:

  sequence     one mvs_fuse_sequence over the 16 references, rows left on the device (one host synchronisation)
  per_view     16 calls of mvs_fuse_depth on the same store, rows left on the device (16 host synchronisations)
  masked       one mvs_fuse_depth_masked (min_support 2 on planes drawn from 0..4) and, beside it, unmasked: one mvs_fuse_depth of that reference

each by the host clock around the call (every call ends in a stream synchronisation) and by HIP events (mvs_profile_read(MVS_K_FUSE): the
launches of the call, without the read-back), medians over --iters repetitions after --warmup.  A measurement path that finds no GPU fails.

One run, under its own time limit (--limit seconds: the process ends itself when it is over).

    python tools/time_fuse_sequence.py [--iters 30] [--warmup 5] [--limit 300] [--out profiles/fuse_sequence/times.json]
"""
import argparse
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mesh-reconstruction_amd", "python"))
import numpy as np  # noqa: E402

import mvs_amd  # noqa: E402
from mvs_amd import synth  # noqa: E402

NREF, K, RING, MIN_SUPPORT = 16, 4, 0.15, 2


def _timed(ctx, call):
    """(host ms, event ms) of one call"""
    ctx.profile_read(reset=True)
    t0 = time.perf_counter()
    call()
    wall = (time.perf_counter() - t0) * 1e3
    ms, _ = ctx.profile_read(reset=True)
    return wall, ms[mvs_amd.MVS_K_FUSE]


def _single(ctx, ref, nbrs, min_support=0):
    """mvs_fuse_depth / mvs_fuse_depth_masked with the rows left on the device -> row count"""
    nb = np.ascontiguousarray(nbrs, np.int32)
    n = mvs_amd.C.c_int(0)
    p = nb.ctypes.data_as(mvs_amd._i32p)
    if min_support:
        rc = ctx.lib.mvs_fuse_depth_masked(ctx.h, ref, len(nb), p, 2, 1.0, 0.01, float("inf"), min_support, None, mvs_amd.C.byref(n))
    else:
        rc = ctx.lib.mvs_fuse_depth(ctx.h, ref, len(nb), p, 2, 1.0, 0.01, float("inf"), None, mvs_amd.C.byref(n))
    if rc:
        raise mvs_amd.MvsError(ctx.lib.mvs_last_error(ctx.h).decode())
    return n.value


def one(W, H, iters, warmup):
    scene = synth.Scene(freq_scale=W / 1920.0)
    rng = np.random.Generator(np.random.PCG64(0x5E9 + W))
    centres = [(RING * np.cos(a), RING * np.sin(a), 0.0) for a in 2 * np.pi * np.arange(NREF) / NREF]
    refs = list(range(NREF))
    lists = [[(i + d) % NREF for d in (-2, -1, 1, 2)] for i in refs]
    with mvs_amd.Context(W, H) as ctx:
        ctx.depth_store(NREF)
        for s, c in enumerate(centres):
            ctx.depth_upload(s, synth.camera_at(c, W, H), scene.render(c, W, H, want_depth=True)[1])
            ctx.depth_support_upload(s, rng.integers(0, 5, (H, W), dtype=np.uint8))
        _, counts = ctx.fuse_sequence(refs, lists, max_rows=0, copy=False)
        total = int(counts.sum())
        each = [_single(ctx, i, lists[i]) for i in refs]
        masked_rows = _single(ctx, 0, lists[0], MIN_SUPPORT)
        arms = {
            "sequence": lambda: ctx.fuse_sequence(refs, lists, max_rows=total, copy=False),
            "per_view": lambda: [_single(ctx, i, lists[i]) for i in refs],
            "masked": lambda: _single(ctx, 0, lists[0], MIN_SUPPORT),
            "unmasked": lambda: _single(ctx, 0, lists[0]),
        }
        ctx.profile_enable(True)
        times = {name: [] for name in arms}
        for it in range(warmup + iters):
            for name, call in arms.items():   # alternating: every repetition runs all four
                t = _timed(ctx, call)
                if it >= warmup:
                    times[name].append(t)
        ctx.profile_enable(False)
    med = {name: np.median(np.asarray(v), axis=0) for name, v in times.items()}
    spread = {name: np.percentile(np.asarray(v)[:, 0], [10, 90]) for name, v in times.items()}
    rec = {"size": "%dx%d" % (W, H), "references": NREF, "neighbours": K, "iters": iters, "warmup": warmup,
           "rows_sequence": total, "rows_per_view_total": int(sum(each)), "rows_masked_single": masked_rows, "rows_unmasked_single": each[0]}
    for name in arms:
        rec[name + "_host_ms"] = round(float(med[name][0]), 4)
        rec[name + "_event_ms"] = round(float(med[name][1]), 4)
        rec[name + "_host_ms_p10_p90"] = [round(float(x), 4) for x in spread[name]]
    rec["sequence_over_per_view_host"] = round(rec["sequence_host_ms"] / rec["per_view_host_ms"], 4)
    rec["sequence_over_per_view_event"] = round(rec["sequence_event_ms"] / rec["per_view_event_ms"], 4)
    rec["masked_over_unmasked_host"] = round(rec["masked_host_ms"] / rec["unmasked_host_ms"], 4)
    rec["masked_over_unmasked_event"] = round(rec["masked_event_ms"] / rec["unmasked_event_ms"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_sequence", "times.json"))
    ap.add_argument("--limit", type=int, default=300)
    a = ap.parse_args()
    signal.alarm(a.limit)   # SIGALRM's default action ends the process
    recs = []
    for W, H in ((640, 480), (1920, 1080)):
        r = one(W, H, a.iters, a.warmup)
        print(json.dumps(r), flush=True)
        recs.append(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
