"""Random call orders over the stages of the sweep family on ONE long-lived context -- every sweep, selection, aggregation, window,
cleaning, the band calls, plane tables, samplers, volume sources, a caller's volume -- against the shadow context (tests/shadow_context.py,
DESIGN.md section 30): after every step everything that can be fetched equals the shadow's bits and everything else returns the promised
code.  Not part of the suite proper (tests/test_shadow_gpu.py runs three seeds of 40 steps):
python tests/perf/fuzz_stages.py [first_seed] [count] [steps per seed]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "mesh-reconstruction_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("MVS_TEST_HOOKS", "1")
import torch  # noqa: F401 (HIP runtime first)
import shadow_context as sc


def run(seed, steps, name="crafted", verbose=False):
    """-> 0, or 1 and the message of the first step that differs"""
    calls = sc.walk_prologue(name) + sc.walk_calls(name, seed, steps)
    shadow, device = sc.Shadow(name), sc.Device(name)
    try:
        for c in calls:
            rc = sc.step(shadow, device, *c)
            if verbose:
                print("seed %d: %s -> %d" % (seed, c, rc), flush=True)
    except AssertionError as e:
        print("seed %d: %s" % (seed, e), flush=True)
        return 1
    finally:
        device.close()
    return 0


if __name__ == "__main__":
    first = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    count = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 40
    total = sum(run(s, steps) for s in range(first, first + count))
    print("stage fuzz: seeds %d..%d x %d steps, %d walks differ from the shadow context" % (first, first + count - 1, steps, total))
