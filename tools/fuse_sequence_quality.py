"""The second quality figure of DESIGN.md section 28, on the GPU: section 27's estimated maps with their support stored for all five views
of the occluder scene (tests/fuse_sequence_cases.py: occluder_sequence_quality), the sequence cloud unmasked and masked by support >= 1..4
of 4, and per cloud its rows and the share of rows more than 1.5 steps of a 48-plane table off.  Prints markdown and writes the figures.

    python tools/fuse_sequence_quality.py [--out profiles/fuse_sequence/quality.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mesh-reconstruction_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fuse_sequence_cases as sc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_sequence", "quality.json"))
    a = ap.parse_args()
    q = sc.occluder_sequence_quality((0, 1, 2, 3, 4))
    print("| occluder, five views, estimated maps | rows | per reference | rows more than 1.5 steps off |")
    print("|---|---|---|---|")
    for ms, r in q.items():
        print("| %s | %d | %s | %.2f %% |" % ("unmasked" if ms == 0 else "support >= %d of 4" % ms, r["rows"], " / ".join(str(c) for c in r["counts"]), r["bad_share"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({str(ms): r for ms, r in q.items()}, f, indent=1)


if __name__ == "__main__":
    main()
