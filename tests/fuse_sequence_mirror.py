"""numpy restatement of the support planes' rule 1s, mvs_fuse_depth_masked, mvs_tsdf_integrate_masked and mvs_fuse_sequence (csrc/fuse.hip,
csrc/tsdf.hip, csrc/fuse_sequence.hip; the contract: DESIGN.md section 28, include/mvs.h).

Rule 1s is the same as overwriting the stored depth with the empty value 1.0 wherever the support is too low: masked() does that, and
fuse_masked / integrate_masked are the existing mirrors (tests/fuse_mirror.py, tests/tsdf_mirror.py, tests/appearance_mirror.py) on the
overwritten maps.  fuse_sequence restates S1-S5 on top of fuse_mirror.fuse: the agreement of every neighbour comes from its `tests`
intermediates, rule 3's pixel is recomputed with fuse_mirror's own _prow statements.  Everything is float32 with one rounding per
operation, so rows, counts and claim planes are expected bit for bit.
"""
import numpy as np

import fuse_mirror as fm
import tsdf_mirror as tm

f32 = np.float32


def masked(depths, supports, min_support):
    """depths: slot -> [H, W]; supports: slot -> [H, W] u8 -> the maps with 1.0 wherever the slot's support is below min_support (> 0)"""
    if min_support <= 0:
        return dict(depths)
    out = {}
    for s, d in depths.items():
        d = np.array(d, f32)
        if s in supports:
            d[np.asarray(supports[s]).astype(np.int64) < min_support] = f32(1.0)
        out[s] = d
    return out


def fuse_masked(depths, costs, supports, mats, ref, neighbours, min_support=0, **kw):
    """mvs_fuse_depth_masked: fuse_mirror.fuse on the overwritten maps"""
    return fm.fuse(masked(depths, supports, min_support), costs, mats, ref, list(neighbours), **kw)


def integrate_masked(vol, depths, costs, supports, mats, slots, min_support=0, max_cost=np.inf, frames=None, frame_slots=None):
    """mvs_tsdf_integrate_masked into a tsdf_mirror.Volume (frame_slots None) or an appearance_mirror.Volume: the w-maps of the
    overwritten maps, then the existing integration"""
    md = masked({s: depths[s] for s in set(slots)}, supports, min_support)
    maps = {s: tm.wmap(md[s], costs[s] if max_cost < np.inf else None, mats[s], max_cost) for s in md}
    if frame_slots is None:
        return vol.integrate(maps, mats, list(slots))
    return vol.integrate_frames(maps, mats, frames, list(zip(slots, frame_slots)))


def vote_pixel(P, X, W, H):
    """rule 3's pixel (row, col) of the points X [H, W, 3] in the view with matrix P, and whether there is one"""
    P = np.asarray(P, f32)
    Xc = (X[..., 0], X[..., 1], X[..., 2])
    halfW, halfH = f32(W) * f32(0.5), f32(H) * f32(0.5)
    with np.errstate(all="ignore"):
        qw = fm._prow(P, 3, Xc)
        u = (fm._prow(P, 0, Xc) / qw + f32(1.0)) * halfW - f32(0.5)
        v = (f32(1.0) - fm._prow(P, 1, Xc) / qw) * halfH - f32(0.5)
        fc, fr = np.floor(u + f32(0.5)), np.floor(v + f32(0.5))
        inb = (qw > f32(0.0)) & (fc >= f32(0.0)) & (fc < f32(W)) & (fr >= f32(0.0)) & (fr < f32(H))
    return np.where(inb, fr, 0).astype(np.int64), np.where(inb, fc, 0).astype(np.int64), inb


def fuse_sequence(depths, costs, supports, mats, refs, neighbours, min_consistent=2, max_reproj_px=1.0, max_rel_depth=0.01, max_cost=np.inf,
                  min_support=0, max_rows=None):
    """refs: the reference slots in order; neighbours: one list per reference (-1 = none).  Returns a dict: rows (the first max_rows of
    them), total, counts per reference, claims {slot: [H, W] u8}, and per reference kept (the pixels that started a point), shadowed (kept by
    rules 1s-5 but claimed), agreed ({position in its list: the pixels that neighbour agreed at}), before ({neighbour: its claim plane when the
    turn began}), wrote ({neighbour: the pixels of its plane this turn stored a 1 at}) and res (fuse_mirror.fuse's result)."""
    md = masked(depths, supports, min_support)
    H, W = np.asarray(depths[refs[0]]).shape
    reproj2 = f32(max_reproj_px) * f32(max_reproj_px)
    slots = sorted(set(refs) | {j for row in neighbours for j in row if j != -1})
    claim = {s: np.zeros((H, W), np.uint8) for s in slots}   # S1
    rows, counts, per_ref = [], [], []
    for ref, row in zip(refs, neighbours):   # S2: in list order
        nbrs = [j for j in row if j != -1]
        maps = md   # claims gate nothing else: tangents and votes read the maps as they are
        res = fm.fuse(maps, costs, mats, ref, nbrs, min_consistent=min_consistent, max_reproj_px=max_reproj_px, max_rel_depth=max_rel_depth, max_cost=max_cost)
        kept = res["keep"] & (claim[ref] == 0)
        before = {j: claim[j].copy() for j in set(nbrs)}
        agreed, wrote = {}, {j: np.zeros((H, W), bool) for j in set(nbrs)}
        for k, (j, (reached, d2, rel)) in enumerate(zip(nbrs, res["tests"])):   # S3
            with np.errstate(all="ignore"):
                agreed[k] = reached & (d2 <= reproj2) & (rel <= f32(max_rel_depth))
            rj, cj, _ = vote_pixel(mats[j][0], res["X"], W, H)
            sel = kept & agreed[k]
            claim[j][rj[sel], cj[sel]] = 1
            wrote[j][rj[sel], cj[sel]] = True
        rows.append(res["rows"][kept[res["keep"]]])   # S4: ascending pixel index within the reference
        counts.append(int(kept.sum()))
        per_ref.append({"ref": ref, "nbrs": nbrs, "kept": kept, "shadowed": res["keep"] & (claim[ref] != 0), "agreed": agreed, "res": res,
                        "before": before, "wrote": wrote})
    rows = np.concatenate(rows) if rows else np.zeros((0, 7), f32)
    total = len(rows)
    if max_rows is not None:
        rows = rows[:max_rows]
    return {"rows": rows.astype(f32), "total": total, "counts": np.asarray(counts, np.int32), "claims": claim, "per_ref": per_ref}
