"""The quality tables of DESIGN.md section 27, computed with the mirror (tests/consistency_mirror.py) on the CPU: section 25's setup on
section 22's occluder scene and section 26's contrast scene (160 x 100, 4 side views, ZNCC r = 2, keep 2, 3 iterations without random
candidates from the 16-plane map; bad = more than 1.5 steps of a 48-plane table off; cap 3 px), with the neighbours' maps analytic or
estimated by the same recipe, and the support mask's table (cap 1 px).  Prints markdown; takes a few minutes.

    python tools/consistency_quality.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mesh-reconstruction_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import consistency_cases as cc  # noqa: E402
import gated_cases as gc  # noqa: E402
import orc  # noqa: E402

ROWS = (("occluder", 255, "analytic"), ("contrast", 255, "analytic"), ("occluder", 255, "estimated"), ("occluder", 30, "estimated"), ("contrast", 255, "estimated"))


def main():
    oracle = orc.load()
    fmt = lambda s: "%.2f / %.2f" % s
    print("| scene, gate, neighbour maps | start | photometric | + term, w 2.5 | + term, w 10 |")
    print("|---|---|---|---|---|")
    for name, tau, nb in ROWS:
        shares = lambda z: gc.bad_shares(oracle, name, z, 48)
        cells = [fmt(shares(gc.propagation_start(name))) if tau == 255 else "–", fmt(shares(gc.propagated(name, tau, False)))]
        cells += [fmt(shares(cc.consistent(name, nb, w, 3.0, tau)[0])) for w in (2.5, 10.0)]
        print("| %s, tau %d, %s | %s |" % (name, tau, nb, " | ".join(cells)), flush=True)
    s = gc.scene("occluder")
    z, support = cc.consistent("occluder", "estimated", 10.0, 1.0, 255)
    bad = np.abs(z - s.truth) > 1.5 * (s.z_hi - s.z_lo) / 48
    print()
    print("| occluder, tau 255, estimated neighbours, w 10, cap 1 px | pixels kept | bad among them | bad among their edge pixels |")
    print("|---|---|---|---|")
    for least in (0, 1, 2, 3, 4):
        keep = support >= least
        print("| support >= %d of 4 | %.1f %% | %.2f %% | %.2f %% |" % (least, 100.0 * keep.mean(), 100.0 * bad[keep].mean(), 100.0 * bad[keep & s.edge].mean()), flush=True)


if __name__ == "__main__":
    main()
