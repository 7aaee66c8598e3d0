"""numpy restatement of the 6-nearest-neighbour spacing search of csrc/poisson.hip AS IT WAS BEFORE the shell scan (the parent rule), kept
as the record of what tests/poisson_cases.py's budget cloud is built against: the list of nearest distances was reset at the start of
every pass over R, and a budget that ran out in the middle of a pass left only what the scanned part of that pass had found.  The
cell grid and the sort are the library's as they still are (float64 host arithmetic on the float32 quotients, float32 on the device).
TEST INFRASTRUCTURE ONLY; no GPU."""
import numpy as np

KNN = 6
KNN_BUDGET = 1 << 17
KNN_ROW_COST = 16
F = np.float32


def cell_grid(points):
    """the uniform grid the host code lays over the 2nd .. 98th percentile of the samples -> dict(ox, oy, oz, inv, cell: float32; nx, ny, nz)"""
    p = np.asarray(points, np.float32)
    q = (p[:, :3] / p[:, 3:4]).astype(np.float32)
    n = len(q)
    a, b = int(0.02 * (n - 1)), int(0.98 * (n - 1))
    srt = np.sort(q, axis=0).astype(np.float64)
    rlo, rhi = srt[a], srt[b]
    rside = float((rhi - rlo).max())
    if not rside > 0.0:
        rlo, rhi = srt[0], srt[-1]
        rside = float((rhi - rlo).max())
    cell = max(2.0 * rside / np.sqrt(float(n)), rside / 1000.0)
    dims = [max(1, min(1024, int(np.floor((rhi[c] - rlo[c]) / cell)) + 5)) for c in range(3)]
    return dict(ox=F(rlo[0] - 2.0 * cell), oy=F(rlo[1] - 2.0 * cell), oz=F(rlo[2] - 2.0 * cell), inv=F(1.0 / cell), cell=F(cell), nx=dims[0], ny=dims[1], nz=dims[2])


def cells_of(g, q):
    """cell_of: float32 arithmetic, clamped into the grid -> (i, j, k) int64 arrays"""
    q = np.asarray(q, np.float32).reshape(-1, 3)
    out = []
    for c, (o, m) in enumerate(((g["ox"], g["nx"]), (g["oy"], g["ny"]), (g["oz"], g["nz"]))):
        out.append(np.clip(np.floor((q[:, c] - o) * g["inv"]).astype(np.int64), 0, m - 1))
    return out


def sort_by_cell(points):
    """-> (grid, keys ascending (uint32 as int64), sorted float32 xyz, ids: sorted row -> sample); the device's radix sort is stable"""
    p = np.asarray(points, np.float32)
    q = (p[:, :3] / p[:, 3:4]).astype(np.float32)
    g = cell_grid(p)
    i, j, k = cells_of(g, q)
    keys = (k * g["ny"] + j) * g["nx"] + i
    ids = np.argsort(keys, kind="stable")
    return g, keys[ids], q[ids], ids


def parent_search(g, keys, q, s):
    """the parent kernel's thread for sorted row s -> (value float32, dict(budget: what is left, R: the last pass, found: neighbours used))"""
    p = q[s]
    ci, cj, ck = (int(v[0]) for v in cells_of(g, p))
    rmax = max(g["nx"], g["ny"], g["nz"])
    budget = KNN_BUDGET
    R = 1
    while True:
        best = np.full(KNN, F(3.0e38), np.float32)
        i0, i1 = max(ci - R, 0), min(ci + R, g["nx"] - 1)
        ks = np.arange(max(ck - R, 0), min(ck + R, g["nz"] - 1) + 1)
        js = np.arange(max(cj - R, 0), min(cj + R, g["ny"] - 1) + 1)
        rows = ((ks[:, None] * g["ny"] + js[None, :]) * g["nx"]).ravel()
        lo = np.searchsorted(keys, rows + i0, side="left")
        hi = np.searchsorted(keys, rows + i1 + 1, side="left")
        for a, b in zip(lo.tolist(), hi.tolist()):
            if best[KNN - 1] == 0.0 or budget <= 0:
                b = a
            budget -= (b - a) + KNN_ROW_COST
            if b > a:
                t = np.arange(a, b)
                t = t[t != s]
                d = (q[t] - p).astype(np.float32)
                d2 = ((d[:, 0] * d[:, 0]).astype(np.float32) + (d[:, 1] * d[:, 1]).astype(np.float32)).astype(np.float32)
                d2 = (d2 + (d[:, 2] * d[:, 2]).astype(np.float32)).astype(np.float32)
                best = np.sort(np.concatenate([best, d2]))[:KNN]       # the ascending list of the KNN smallest, whatever the order of arrival
        reach = F(F(R) * g["cell"])
        if best[KNN - 1] <= F(reach * reach) or R >= rmax or budget <= 0:
            break
        R *= 2
    found = best[best < F(3.0e38)]
    total = F(0.0)
    for d2 in found:
        total = F(total + np.sqrt(d2, dtype=np.float32))
    value = F(total / F(len(found) + 1)) if len(found) else F(0.0)
    return value, dict(budget=budget, R=R, found=len(found))
