"""Time the guide-gated windows (csrc/bestk_gated.hip and the gate of csrc/propagate.hip) beside their ungated
counterparts, in one process, after warm-up.

The two cases of tools/time_band.py: 640 x 480 x 4 views on the cameras of the bundled zatisi.yaml (noise frames) and 1920 x 1080 x 16
views of the synthetic scene on ring cameras turned by 0.012 rad.  In each, ZNCC at radius 2 with keep 2, the guide the staged main image:
  (1, 2) mvs_sweep_run_bestk_gated at tau 30 and at tau 255 against mvs_sweep_run_bestk, 32 planes, volume and selection (the gate costs
         the same at every tau: the members are bits; both are recorded).  Radius 4 is timed beside it at the same settings.
  (3)    one iteration of the propagation, mvs_propagate_run(1, dz = half a coarse step, dg = an eighth, nrandom = 2), after an init under
         the gate tau 30 against one after an init under the default gate, from the refined map of a 16-plane mvs_sweep_run_bestk.
All are HIP-event times of the launches (mvs_profile_read: MVS_K_SWEEP), one reading per call, after three warm-up calls.  The variants
are timed in turn and the whole turn is repeated --passes times, so that a drift of the machine falls on all of them; the figure is the
median of passes x iters readings (20 by default) with the minimum and maximum beside it, and the ratio of the medians, gated over
ungated.  There is no gate on the times.  One JSON line per case; --out FILE writes the list.

    python tools/time_gated.py [--iters 10] [--passes 2] [--out profiles/gated/times.json]
"""
import argparse
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mesh-reconstruction_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402  (the HIP runtime first)

import mvs_amd  # noqa: E402
from time_band import cases, kernel_ms, spread  # noqa: E402

BOTH = mvs_amd.MVS_SWEEP_VOLUME | mvs_amd.MVS_SWEEP_FUSED_ARGMIN
ZNCC = mvs_amd.MVS_COST_ZNCC
COARSE, PLANES, KEEP, TAU, NRANDOM = 16, 32, 2, 30, 2


def one(name, W, H, main_cam, main_img, side_cams, sides, iters, passes):
    V = len(sides)
    step = 2.0 / COARSE
    rec = {"case": name, "size": "%dx%d" % (W, H), "views": V, "cost": "zncc", "keep": KEEP, "tau": TAU, "planes": PLANES, "nrandom": NRANDOM, "iters": iters,
           "passes": passes, "date": datetime.date.today().isoformat()}
    with mvs_amd.Context(W, H) as ctx:
        rec["device"] = ctx.info()
        ctx.sweep_set(main_cam, main_img, side_cams, sides, COARSE)
        ctx.sweep_run_bestk(ZNCC, 2, KEEP, 0, V, BOTH)
        ctx.sweep_refine_depth()
        start = torch.as_tensor(ctx.depth_device_array(), device="cuda").clone()
        torch.cuda.synchronize()
        ctx.sweep_set_planes(PLANES, -1.0, 1.0)

        def init(tau):
            ctx.propagate_set_gate(tau)
            ctx.propagate_init(start.data_ptr(), ZNCC, 2, KEEP)
            ctx.propagate_set_gate(255)

        def iteration():
            ctx.propagate_run(1, 0.5 * step, 0.125 * step, NRANDOM, 0)

        variants = []
        for r in (2, 4):
            variants += [("bestk_r%d" % r, None, lambda r=r: ctx.sweep_run_bestk(ZNCC, r, KEEP, 0, V, BOTH)),
                         ("gated_r%d_tau_%d" % (r, TAU), None, lambda r=r: ctx.sweep_run_bestk_gated(ZNCC, r, KEEP, TAU, None, 0, V, BOTH)),
                         ("gated_r%d_tau_255" % r, None, lambda r=r: ctx.sweep_run_bestk_gated(ZNCC, r, KEEP, 255, None, 0, V, BOTH))]
        variants += [("iteration_ungated", lambda: init(255), iteration), ("iteration_tau_%d" % TAU, lambda: init(TAU), iteration)]
        ms = {key: [] for key, _, _ in variants}
        for _ in range(passes):
            for key, before, call in variants:       # (an arm's iterations follow its own init)
                if before:
                    before()
                ms[key] += kernel_ms(ctx, call, iters)
        for key in ms:
            rec[key] = {"ms": spread(ms[key])}
        for r in (2, 4):
            base = rec["bestk_r%d" % r]["ms"]["median"]
            for key in ("gated_r%d_tau_%d" % (r, TAU), "gated_r%d_tau_255" % r):
                rec[key]["over_ungated"] = round(rec[key]["ms"]["median"] / base, 3)
        rec["iteration_tau_%d" % TAU]["over_ungated"] = round(rec["iteration_tau_%d" % TAU]["ms"]["median"] / rec["iteration_ungated"]["ms"]["median"], 3)
        # the same cells: tau 255 is the ungated sweep
        ctx.sweep_run_bestk(ZNCC, 2, KEEP, 0, V, mvs_amd.MVS_SWEEP_VOLUME)
        ungated = ctx.sweep_fetch(want_volume=True)[3]
        ctx.sweep_run_bestk_gated(ZNCC, 2, KEEP, 255, None, 0, V, mvs_amd.MVS_SWEEP_VOLUME)
        rec["tau_255_equals_ungated"] = bool((ctx.sweep_fetch(want_volume=True)[3] == ungated).all())
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    recs = [one(*c, a.iters, a.passes) for c in cases()]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
