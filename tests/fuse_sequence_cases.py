"""Inputs shared by tests/test_fuse_sequence_cpu.py (premises on the mirror alone) and tests/test_fuse_sequence_gpu.py (the library against
the mirror, bit for bit): support planes for the stores of tests/fusion_cases.py and the sequence-fusion cases.

The store is fusion_cases.store(W, H): eight general cameras on a scene with a depth step and a ball, at SIZES = 131 x 67 (two 64-column
tiles and a remainder), 64 x 4 (one tile) and 67 x 45 (odd both ways).  Support planes take the values 0..4; MIN_SUPPORT = 2, so 2 sits ON
the threshold and 1 one below it.
"""
import functools

import numpy as np

import fusion_cases as fc

f32 = np.float32
SIZES = fc.SIZES
SEQ_SIZES = [fc.SIZES[0], fc.SIZES[2]]
MIN_SUPPORT = 2
ALL_ZERO, ALL_255 = fc.MIRRORED, fc.CUT   # the two constant planes


@functools.lru_cache(maxsize=None)
def planes(W, H):
    """-> [DEPTH_CAP] support planes [H, W] u8 (read-only).  Per slot: 4 everywhere, then a sprinkle of single pixels drawn from 0..4, then
    blocks of one value each (0, 1, 2, 3 in turn) that straddle the 64-column seams, the 4-row seams and the four image borders; slot
    ALL_ZERO is all 0 and slot ALL_255 all 255"""
    rng = np.random.Generator(np.random.PCG64(0x5EC + 1000 * W + H))
    out = []
    for s in range(fc.DEPTH_CAP):
        p = np.full((H, W), 4, np.uint8)
        draw = rng.random((H, W)) < 0.2
        p[draw] = rng.integers(0, 5, int(draw.sum()), dtype=np.uint8)
        value = s   # the blocks' values rotate with the slot, so that every value meets every seam in some slot
        corners = []
        for c0 in (61, 125, 0, W - 5):          # columns c0 .. c0 + 5: across a seam between c0 + 2 and c0 + 3; the two borders
            for r0 in (2, H // 2 - 1, H - 4):   # rows r0 .. r0 + 4: across a 4-row seam; the last rows
                corners.append((max(r0, 0), max(c0, 0)))
        for r0 in (0, H - 3):
            for c0 in (20, W // 2):
                corners.append((max(r0, 0), c0))
        for r0, c0 in corners:
            if c0 >= W or r0 >= H:
                continue
            p[r0:r0 + 5, c0:c0 + 6] = value % 4
            value += 1
        if s == ALL_ZERO:
            p[:] = 0
        if s == ALL_255:
            p[:] = 255
        p.setflags(write=False)
        out.append(p)
    return out


def supports(W, H):
    return dict(enumerate(planes(W, H)))


# ---- masked single-reference fusion: (name, reference, neighbours, parameters) ------------------------------------------------------------------
MASKED_CASES = [
    ("rolled_votes", fc.ROLLED, [fc.TILTED, fc.WIDE, fc.DEEP, fc.SHIFTED], dict(min_consistent=2)),
    ("tilted_cost", fc.TILTED, [fc.AXIS, fc.ROLLED, fc.WIDE, ALL_ZERO, ALL_255], dict(min_consistent=2, max_cost=float(fc.MAX_COST))),
    ("holey_alone", fc.HOLEY_AXIS, [], dict(min_consistent=0)),
]

# ---- the sequence: the voting cameras as references in two orders, ragged lists, a -1 in the middle, one neighbour listed twice ------------------
ORDERS = {"a": [fc.TILTED, fc.ROLLED, fc.WIDE, fc.DEEP, fc.SHIFTED], "b": [fc.SHIFTED, fc.WIDE, fc.TILTED, fc.DEEP, fc.ROLLED]}
NEIGHBOURS = {fc.TILTED: [fc.ROLLED, fc.WIDE, fc.AXIS, fc.SHIFTED],
              fc.ROLLED: [fc.TILTED, fc.DEEP, fc.SHIFTED],
              fc.WIDE: [fc.TILTED, fc.ROLLED, fc.DEEP, fc.SHIFTED, fc.ROLLED],   # ROLLED votes twice
              fc.DEEP: [fc.WIDE, fc.SHIFTED, fc.MIRRORED, fc.TILTED],
              fc.SHIFTED: [fc.TILTED, -1, fc.WIDE, fc.DEEP]}
SEQ_KW = dict(min_consistent=2, max_reproj_px=1.0, max_rel_depth=0.01)


def padded(order):
    """the order's neighbour lists as the C entry point takes them: [nrefs, 5] int32, -1 = none"""
    out = np.full((len(order), 5), -1, np.int32)
    for i, ref in enumerate(order):
        out[i, :len(NEIGHBOURS[ref])] = NEIGHBOURS[ref]
    return out


def lists(order):
    return [list(NEIGHBOURS[ref]) for ref in order]


_CACHE = {}


def expected(size, order, min_support, mats, tag):
    """the mirror's result of the sequence case; tag names the matrices (host / device) for the cache"""
    import fuse_sequence_mirror as sm
    key = (size, order, min_support, tag)
    if key not in _CACHE:
        st = fc.store(*size)
        _CACHE[key] = sm.fuse_sequence(dict(enumerate(st["depths"])), dict(enumerate(st["costs"])), supports(*size), mats, ORDERS[order], lists(ORDERS[order]),
                                       min_support=min_support, **SEQ_KW)
    return _CACHE[key]


# ---- quality on the occluder scene: estimated maps with their support (DESIGN.md sections 27 and 28) --------------------------------------------
QUALITY_MIN_SUPPORT = 3   # of 4 neighbours, section 27's mask


def occluder_sequence_quality(min_supports=(0, QUALITY_MIN_SUPPORT)):
    """tools/consistency_quality.py's recipe for every view of the occluder scene (160 x 100, the main view and its four side views, each
    estimated with the other four beside it): mvs_amd.propagate_two_stage(support=True) with ZNCC r = 2, keep 2, 16 coarse planes, 3
    iterations without random candidates, the term at weight 10 and cap 1 px; then Context.fuse_sequence over the five second-stage slots
    (min_consistent 2, 1 px, 0.01) per min_support.  A row is bad when its NDC depth in the view that started it is more than 1.5 steps of
    a 48-plane table from that view's analytic depth at the pixel it projects to.  Needs a GPU.
    -> {min_support: dict(rows=, counts=, bad=, bad_share=)}"""
    import gated_cases as gc
    import mvs_amd

    s = gc.scene("occluder")
    W, H, n = s.W, s.H, s.V + 1
    centres = [[0.0, 0.0, 0.0]] + [[s.RING * np.cos(2.0 * np.pi * v / s.V), s.RING * np.sin(2.0 * np.pi * v / s.V), 0.0] for v in range(s.V)]
    cams = [np.asarray(s.main_cam, f32)] + [np.asarray(c, f32) for c in s.side_cams]
    imgs = [s.main_img] + list(s.sides)
    truths = [s.render(c)[1] for c in centres]
    side_slots = [[j for j in range(n) if j != i] for i in range(n)]
    side_cams_of = [np.stack([cams[j] for j in range(n) if j != i]) for i in range(n)]
    limit = 1.5 * (s.z_hi - s.z_lo) / 48
    out = {}
    with mvs_amd.Context(W, H, 0, sampler="fixed") as ctx:
        ctx.frame_store(n)
        for i in range(n):
            ctx.frame_upload(i, imgs[i])
        ctx.depth_store(2 * n)
        mvs_amd.propagate_two_stage(ctx, list(range(n)), np.stack(cams), side_slots, np.stack(side_cams_of), 16, s.z_lo, s.z_hi,
                                    cost=dict(cost="zncc", radius=2, keep=2), propagate=dict(iterations=3, dz_steps=0.0, dg_steps=0.0, nrandom=0, seed=0),
                                    consistency=dict(weight=10.0, max_px=1.0), fetch=False, support=True)
        refs = [n + i for i in range(n)]
        lists = [[r for r in refs if r != ref] for ref in refs]
        for ms in min_supports:
            rows, counts = ctx.fuse_sequence(refs, lists, min_consistent=2, max_reproj_px=1.0, max_rel_depth=0.01, min_support=ms)
            bad, at = 0, 0
            for i, c in enumerate(counts):
                X = rows[at:at + c, :3].astype(np.float64)
                at += c
                P = cams[i].astype(np.float64)
                q = X @ P[:, :3].T + P[:, 3]
                col = np.clip(np.floor((q[:, 0] / q[:, 3] + 1.0) * W / 2.0).astype(np.int64), 0, W - 1)
                row = np.clip(np.floor((1.0 - q[:, 1] / q[:, 3]) * H / 2.0).astype(np.int64), 0, H - 1)
                bad += int((np.abs(q[:, 2] / q[:, 3] - truths[i][row, col]) > limit).sum())
            out[ms] = dict(rows=int(len(rows)), counts=[int(c) for c in counts], bad=bad, bad_share=100.0 * bad / max(len(rows), 1))
    return out
