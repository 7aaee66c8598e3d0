"""numpy restatement of the map-cleaning contract, written from the contract and not from the kernels.

Integers only (int64 work arrays: the largest product, s n 100 with a 24-bit sum and a 16-bit count, stays below 2^48).  Volumes and S
are [D, H, W]; `cs` is the count shift of the packed cell (24 for the fixed sampler, 16 for the exact one).  Components come from a
plain union-find: the runs of connected pixels of every row are the nodes, the connected pixel pairs of neighbouring rows the edges."""
import numpy as np

BACKGROUND_DEPTH = np.float32(1.0)


def split(vol, cs):
    """packed cells -> (sum, count) as int64"""
    v = np.asarray(vol, np.uint32).astype(np.int64)
    return v & ((1 << cs) - 1), v >> cs


def _at(a, index):
    """a[index[p], p] for every pixel, plane 0 standing in where there is no index"""
    return np.take_along_axis(a, np.clip(index, 0, None)[None].astype(np.int64), axis=0)[0]


def rule1(index, vol, cs, min_views):
    """bool [H, W]: pixels with an index whose selected cell was seen by fewer than min_views views"""
    _, n = split(vol, cs)
    return (index >= 0) & (_at(n, index) < min_views)


def rule2(index, vol, cs, u, S=None):
    """bool [H, W]: pixels with an index that have a seen rival at least 2 planes away with score(d) (100 - u) < score(i) 100;
    the scores are S where it is given, else the cells' mean costs s / n compared as s_d n_i (100 - u) < s_i n_d 100"""
    s, n = split(vol, cs)
    D = s.shape[0]
    d = np.arange(D)[:, None, None]
    far = np.abs(d - index[None]) >= 2
    if S is not None:
        S = np.asarray(S).astype(np.int64)
        less = S * (100 - u) < _at(S, index)[None] * 100
    else:
        less = s * _at(n, index)[None] * (100 - u) < _at(s, index)[None] * n * 100
    return (index >= 0) & (far & (n > 0) & less).any(axis=0)


def _find(parent, x):
    root = x
    while parent[root] != root:
        root = parent[root]
    while parent[x] != root:
        parent[x], x = root, parent[x]
    return root


def component_sizes(index, max_diff):
    """int32 [H, W]: pixel count of the 4-connected component of every pixel (both pixels of a connected pair have an index, and the
    indices differ by at most max_diff; components are the transitive closure), 0 for a pixel without an index"""
    index = np.asarray(index).astype(np.int64)
    H, W = index.shape
    valid = index >= 0
    # nodes: runs of connected pixels along the rows (a pixel without an index is a run of its own and stays out of every edge)
    joined = np.zeros((H, W), bool)
    joined[:, 1:] = valid[:, 1:] & valid[:, :-1] & (np.abs(index[:, 1:] - index[:, :-1]) <= max_diff)
    run = np.cumsum(~joined.ravel()).reshape(H, W) - 1
    parent = list(range(int(run.max()) + 1))
    # edges: connected pairs of neighbouring rows, every pair of runs once
    down = valid[1:] & valid[:-1] & (np.abs(index[1:] - index[:-1]) <= max_diff)
    pairs = np.unique(np.stack([run[:-1][down], run[1:][down]], axis=1), axis=0)
    for a, b in pairs.tolist():
        ra, rb = _find(parent, a), _find(parent, b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    root = np.array([_find(parent, r) for r in range(len(parent))], np.int64)[run]
    count = np.bincount(root[valid], minlength=len(parent))
    return np.where(valid, count[root], 0).astype(np.int32)


def clean(depth, cost, index, vol=None, cs=24, S=None, min_views=0, uniqueness=0, speckle_min_size=0, speckle_max_diff=1):
    """the maps after mvs_sweep_clean -> (depth, cost, index, report, sizes): report = [pixels with an index before, rejected by rule 1,
    2, 3], sizes = the component sizes of the index map rules 1-2 left (None with speckle_min_size 0).  `S`: the scores of rule 2
    (MVS_CLEAN_SCORES_AGGREGATED).  Without a volume only rule 3 can run (min_views <= 1 and uniqueness 0)."""
    assert 0 <= min_views <= 255 and 0 <= uniqueness <= 99 and speckle_min_size >= 0 and 0 <= speckle_max_diff <= 255
    index = np.asarray(index, np.int32)
    valid = int((index >= 0).sum())
    if vol is None:
        assert min_views <= 1 and uniqueness == 0 and S is None
    r1 = rule1(index, vol, cs, min_views) if vol is not None else np.zeros(index.shape, bool)
    r2 = rule2(index, vol, cs, uniqueness, S) & ~r1 if uniqueness else np.zeros(index.shape, bool)   # both on the incoming maps
    index = np.where(r1 | r2, -1, index).astype(np.int32)
    sizes, r3 = None, np.zeros(index.shape, bool)
    if speckle_min_size:
        sizes = component_sizes(index, speckle_max_diff)      # every size before any pixel is rewritten
        r3 = (sizes > 0) & (sizes < speckle_min_size)
    gone = r1 | r2 | r3
    return (np.where(gone, BACKGROUND_DEPTH, depth).astype(np.float32), np.where(gone, np.float32(np.inf), cost).astype(np.float32),
            np.where(gone, -1, index).astype(np.int32), [valid, int(r1.sum()), int(r2.sum()), int(r3.sum())], sizes)
