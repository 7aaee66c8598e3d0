"""The turn of a CLEAN region in the rectified-view sweep kernel (csrc/sweep_rect.hip), read from the compiler's gfx950 listing of the
headline instantiation sweep_fx_rect<84, true, true> (the Makefile's own CXXFLAGS, as tests/test_rect_resources_cpu.py compiles it).

The path looked at: from the region loop's s_barrier to the first ds_read_addtid_b32 of the clean body -- the copy issue for the next
region, the record fetch, the record decode.  Every instruction between the two lines is counted, whichever side of a branch it is on
(the same rule for every build, so two builds compare).  Checked:
  (a) no EXEC masking and no scalar multiply on it: the copies run whole-wavefront under the buffer's range check, and what the
      kernel used to derive per region comes out of the planner's records;
  (b) a ratchet on the scalar and the non-sample vector instructions of the path, and both below what the previous kernel (the one with
      the lane-masked copies and the (chunk, view) cursor) had on the same path, counted by this file's `python tests/test_rect_turn_cpu.py
      <sweep_rect.hip>` (profiles/r08/README.md has both rows).
s_waitcnt, s_nop and s_barrier are not scalar-pipe work and are counted with neither."""
import os
import re
import shlex
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mesh-reconstruction_amd")
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
HEADLINE = "_ZN3mvs13sweep_fx_rectILi84ELb1ELb1EEEvNS_8RectArgsE"

# the previous kernel on this path (this file's main on its csrc/sweep_rect.hip): scalar, vector
PREVIOUS = (81, 26)
# this kernel (the ratchet: an edit may lower these, not raise them)
SCALAR_MAX, VECTOR_MAX = 20, 17

NOT_SALU = ("s_waitcnt", "s_nop", "s_barrier")


def _makefile_flags():
    text = open(os.path.join(PKG, "Makefile")).read()
    m = re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", text, re.M)
    assert m, "no CXXFLAGS line in the Makefile"
    return shlex.split(m.group(1).replace("$(ARCH)", "gfx950"))


def listing(source, workdir):
    """gfx950 assembly of `source` (a sweep_rect.hip; its includes are taken from the package's csrc)"""
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    assert hipcc, "hipcc is needed to compile the kernel"
    out = os.path.join(workdir, "sweep_rect.s")
    r = subprocess.run([hipcc] + _makefile_flags() + ["-I", os.path.join(PKG, "csrc"), "--cuda-device-only", "-S", source, "-o", out],
                       cwd=PKG, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return open(out).read()


def turn_path(asm, kernel=HEADLINE):
    """the instructions between the region loop's s_barrier and the clean body's first ds_read_addtid_b32"""
    lines = asm.splitlines()
    start = lines.index(next(l for l in lines if l.startswith(kernel + ":")))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[start:end]
    first_read = next(i for i, l in enumerate(body) if l.strip().startswith("ds_read_addtid_b32"))
    barrier = max(i for i in range(first_read) if body[i].strip() == "s_barrier")
    ops = []
    for l in body[barrier + 1:first_read]:
        t = l.strip()
        if not t or t.startswith((";", ".", "//")) or t.endswith(":"):
            continue
        ops.append(t.split()[0])
    return ops


def counts(ops):
    scalar = sum(1 for o in ops if o.startswith("s_") and not o.startswith(NOT_SALU))
    vector = sum(1 for o in ops if o.startswith(("v_", "buffer_", "ds_", "global_", "flat_", "scratch_")))
    return scalar, vector


def test_clean_turn_of_the_headline_kernel(tmp_path):
    ops = turn_path(listing(os.path.join("csrc", "sweep_rect.hip"), str(tmp_path)))
    scalar, vector = counts(ops)
    print("clean turn, barrier to first read: %d scalar, %d vector instructions (previous kernel: %d, %d)" % ((scalar, vector) + PREVIOUS))
    for banned in ("s_cbranch_execz", "s_and_saveexec", "s_mul"):
        hits = [o for o in ops if o.startswith(banned)]
        assert not hits, "%s on the clean turn: %s" % (banned, hits)
    assert scalar <= SCALAR_MAX, ops
    assert vector <= VECTOR_MAX, ops
    assert scalar < PREVIOUS[0] and vector < PREVIOUS[1]


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        for src in sys.argv[1:] or [os.path.join(PKG, "csrc", "sweep_rect.hip")]:
            ops = turn_path(listing(os.path.abspath(src), d))
            print(src, "scalar %d vector %d" % counts(ops))
            print("  " + " ".join(ops))
