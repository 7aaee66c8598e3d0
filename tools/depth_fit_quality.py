"""What the depth-map plane fit buys, measured on the CPU through the committed mirrors, which the device equals bit for bit (DESIGN.md
section 32's quality tables).  No GPU is needed.

1. Section 31's table again (section 25's exposure scene at 96 x 64, 16 planes refined, section 25's recipe, the main view fused alone;
   angle of each row's normal to the analytic normal) with three more rows: (a) normals from the fit (r = 4, tau 255, max_step 4 coarse
   plane steps) of the raw refined map, (b) the same fit of the propagated z map, (c) section 25's recipe seeded through the fit's slopes,
   then rule N1; and the share of pixels that still hold their seed's slopes after the three iterations.
2. Section 23's two scenes (48 planes, windowed R = 4, refined): the bad-pixel share of zfit against the gated mean and the filter, the
   same r = 4 and 8-step gate.

    python tools/depth_fit_quality.py [--out profiles/depth_fit/quality.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mesh-reconstruction_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import depth_filter_mirror as dm  # noqa: E402
import depth_fit_cases as fc  # noqa: E402
import depth_fit_mirror as fm  # noqa: E402
import fuse_sequence_mirror as sm  # noqa: E402
import fusion_cases as fuc  # noqa: E402
import normals_mirror as nm  # noqa: E402
import orc  # noqa: E402
import propagate_cases as pc  # noqa: E402
import propagate_mirror as pm  # noqa: E402
import window_mirror as wm  # noqa: E402
from mvs_amd import synth  # noqa: E402
from test_normals_cpu import scene_normal  # noqa: E402

f32 = np.float32


def _figures(rows):
    cos = np.abs((rows[:, 4:7].astype(np.float64) * scene_normal(rows[:, :3])).sum(-1))
    angle = np.degrees(np.arccos(np.clip(cos, 0.0, 1.0)))
    return {"median_deg": round(float(np.median(angle)), 2), "p90_deg": round(float(np.percentile(angle, 90)), 2), "rows": int(len(rows))}


def normals_table(oracle):
    W, H = 96, 64
    views, truth, start = pc.exposure_start(W, H)
    coarse = 2.0 / 16
    scene = pm.Scene(oracle, *views)
    recipe = (3, 0.5 * coarse, 0.125 * coarse, 3, 0)
    mats = {0: fuc.mats32(views[0])}
    P, C = mats[0][0], mats[0][2]
    fuse = lambda depth, normals: _figures(nm.fuse_normals({0: np.asarray(depth, f32)}, {}, {}, {0: normals}, mats, 0, [], min_consistent=0)["rows"])
    out = {}
    state = pm.State(scene, start, pc.ZNCC, 3, pc.KEEP_ALL).run(*recipe)
    out["tangent normals (rule 5)"] = _figures(sm.fuse_masked({0: np.asarray(state.z, f32)}, {}, {}, mats, 0, [], min_consistent=0)["rows"])
    out["slope normals (rule N1), zero seeds"] = dict(fuse(state.z, nm.hypothesis_normals(state.z, state.gx, state.gy, P, C)),
                                                      seed_slopes_held=round(float(((state.gx == 0) & (state.gy == 0)).mean()), 3))
    raw = fm.fit(start, 4, 255, f32(4 * coarse), 6)
    out["(a) fit of the raw refined map"] = dict(fuse(start, fm.normals(raw, P, C)), fitted=round(float((raw.members > 0).mean()), 3))
    prop = fm.fit(state.z, 4, 255, f32(4 * coarse), 6)
    out["(b) fit of the propagated z map"] = dict(fuse(state.z, fm.normals(prop, P, C)), fitted=round(float((prop.members > 0).mean()), 3))
    seeded = fc.seeded_state(scene, start, pc.ZNCC, 3, pc.KEEP_ALL, raw.gx, raw.gy)
    seed_gx, seed_gy = seeded.gx.copy(), seeded.gy.copy()
    seeded.run(*recipe)
    out["(c) recipe seeded through fit=, then rule N1"] = dict(fuse(seeded.z, nm.hypothesis_normals(seeded.z, seeded.gx, seeded.gy, P, C)),
                                                               seed_slopes_held=round(float(((seeded.gx == seed_gx) & (seeded.gy == seed_gy)).mean()), 3))
    step = 1.5 * 2.0 / 48
    for name, z in (("zero seeds", state.z), ("seeded", seeded.z), ("zfit of the propagated map", prop.zfit)):
        err = np.abs(np.asarray(z, np.float64) - truth)
        out["depth, " + name] = {"bad_share": round(float((err > step).mean()), 4), "median_error": round(float(np.median(err)), 5)}
    return out


def zfit_table(oracle):
    out = {}
    for W, H in ((96, 64), (160, 100)):
        main_cam, main_img, side_cams, sides, truth = synth.make_views(W, H, 4)
        lo, hi = float(truth.min()) - 0.01, float(truth.max()) + 0.01
        step = (hi - lo) / 48
        z = oracle.plane_table(48, lo, hi)
        vol = oracle.sweep(main_cam, main_img, side_cams, sides, 48, lo, hi, want_volume=True, nthreads=4, sampler="fixed")[3]
        wv = wm.window(vol, 24, 4)
        sweep = oracle.refine_depth(wv, z, oracle.argmin(wv, z, sampler="fixed")[2], sampler="fixed")
        gate = f32(8.0 * step)
        median = dm.filter(sweep, 4, 255, gate, main_img, dm.MEDIAN)
        maps = {"windowed sweep": sweep, "gated mean": dm.filter(sweep, 4, 255, gate, main_img, dm.MEAN), "median, then mean (section 23's filter)": dm.filter(sweep, 4, 255, gate, main_img),
                "zfit": fm.fit(sweep, 4, 255, gate, 6).zfit, "zfit of the median's map": fm.fit(median, 4, 255, gate, 6).zfit}
        out["%dx%d" % (W, H)] = {k: {"bad_share": round(float((np.abs(m.astype(np.float64) - truth) > 1.5 * step).mean()), 4),
                                     "median_error": round(float(np.median(np.abs(m.astype(np.float64) - truth))), 5)} for k, m in maps.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    oracle = orc.load()
    rec = {"normals on the exposure scene, 96x64": normals_table(oracle), "zfit on section 23's scenes": zfit_table(oracle)}
    print(json.dumps(rec, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
