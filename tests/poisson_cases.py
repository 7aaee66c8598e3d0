"""Crafted inputs for the five device stages of csrc/poisson.hip (tests/test_poisson_cases_cpu.py checks that they reach what they
claim, tests/test_poisson_cases_gpu.py runs them): clouds for the spacing search (compared per sample), clouds for the fixed-point
splat and the level at the smallest grid of the API (16^3 nodes, h = 0.125 and origin = -0.3125 exact), fields and node masks for the
surface nets, weight fields for the support mask.  Everything is deterministic; arrays are built once and handed out read-only."""
import functools

import numpy as np

F = np.float32


def _ro(a):
    a.setflags(write=False)
    return a


def _rows(xyz, w=None):
    """xyzw float32 rows: xyz rounded to float32 first, then multiplied by w (a power of two: the quotient the library forms is exact)"""
    xyz = np.asarray(xyz, np.float32)
    w = np.ones(len(xyz), np.float32) if w is None else np.asarray(w, np.float32)
    return np.concatenate([xyz * w[:, None], w[:, None]], 1).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# spacing clouds
def _unit_sphere(rng, n):
    u = rng.normal(size=(n, 3))
    return (u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def spacing_clouds():
    """name -> xyzw rows.  n = 2 .. 8: fewer neighbours than 6, exactly 6, one more; a lattice (distances tie; its lowest samples sit on a
    border of the cell grid, up to the rounding of the grid's origin); duplicates; homogeneous w of both signs; outliers beyond the cell grid on
    every side of it"""
    out = {}
    rng = np.random.default_rng(2024)
    for n in (2, 3, 6, 7, 8):
        out["n%d" % n] = _rows(rng.uniform(-1.0, 1.0, size=(n, 3)))
    k, j, i = np.meshgrid(np.arange(5), np.arange(5), np.arange(5), indexing="ij")
    out["lattice"] = _rows(np.stack([i, j, k], -1).reshape(-1, 3) * 0.25)
    out["duplicates"] = _rows(np.tile(rng.uniform(0.0, 1.0, size=(64, 3)).astype(np.float32), (8, 1)))
    sphere = _unit_sphere(rng, 2000)
    w = rng.choice(np.array([0.5, 2.0, -1.0, -4.0], np.float32), size=2000)
    out["sphere-w"] = _rows(sphere, w)
    far = np.array([[5, 0, 0], [-5, 0, 0], [0, 5, 0], [0, -5, 0], [0, 0, 5], [0, 0, -5], [5, 5, 5], [-5, -5, -5]], np.float32)
    out["sphere-outliers"] = _rows(np.concatenate([sphere, far]), np.concatenate([w, w[:8]]))
    return {name: _ro(v) for name, v in out.items()}


BUDGET_ROW = 0   # the isolated sample of budget_cloud()


@functools.lru_cache(maxsize=None)
def budget_cloud():
    """250 000 rows, w = 1: row 0 = (0.6, 0.6, 0.02) lies 0.43 below a slab of 239 999 uniform samples and 0.7 from a dense box of 10 000.
    Around it the passes R = 1 .. 32 of the spacing search meet empty cell rows only, and the pass R = 64 spends what is left of the budget
    on empty rows below the slab: the search as it was before the shell scan ended with no neighbour at all and reported 0
    (tests/knn_mirror.py restates it; the exact value is 0.37)."""
    rng = np.random.default_rng(77)
    n, slab = 250000, 239999
    xyz = np.empty((n, 3), np.float64)
    xyz[0] = (0.6, 0.6, 0.02)
    xyz[1:1 + slab] = rng.uniform([0.0, 0.0, 0.45], [1.0, 1.0, 1.0], size=(slab, 3))
    xyz[1 + slab:] = rng.uniform([0.0, 0.0, 0.0], [0.1, 0.1, 0.3], size=(n - 1 - slab, 3))
    return _ro(_rows(xyz))


# ---------------------------------------------------------------------------------------------------------------------------------
# splat and level clouds: mvs_poisson_surface at grid_log2 = 4.  The samples span [0, 1.25]^3 exactly: box = 1.875, h = 1.875 / 15 = 0.125,
# origin = 0.625 - 0.9375 = -0.3125, all exact in float32; node i lies at -0.3125 + 0.125 i, the samples' box spans grid coordinates 2.5 .. 12.5.
SPLAT_G, SPLAT_H, SPLAT_ORIGIN = 16, F(0.125), np.full(3, -0.3125, np.float32)


def _node(i):
    return -0.3125 + 0.125 * i


def _next_up(x):
    return np.nextafter(F(x), F(np.inf))


@functools.lru_cache(maxsize=None)
def splat_cloud():
    """-> (xyzw rows, normal rows).  A trilinear weight is a product of t or 1 - t per axis: 1/8 at the middle of a cell, 1/4 at the middle of
    a cell face, 1 on a node -- so a normal component of (k + 1/2) / (65536 x weight) puts n x weight x 2^16 exactly half-way between two
    integers, and rintf must round it to the even one.  k around 5000 / 10000 / 40000 keeps those components in [0.5, 1): the normals'
    scale stays 2^0 (the lower median of the largest components)."""
    xyz, nrm, w = [], [], []

    def add(p, n, ww=1.0):
        xyz.append(p), nrm.append(n), w.append(ww)

    def tie(k, weight):
        return (k + 0.5) / (65536.0 * weight)

    # the two corners of the samples' box and two more cell centres: weight 1/8 at 8 nodes each; even / odd k, both signs
    add((0.0, 0.0, 0.0), (tie(5000, 0.125), tie(5002, 0.125), tie(6000, 0.125)))
    add((1.25, 1.25, 1.25), (tie(5001, 0.125), tie(5003, 0.125), tie(6001, 0.125)))
    add((0.5, 0.5, 0.5), (-tie(5000, 0.125), -tie(5002, 0.125), -tie(6000, 0.125)), 2.0)
    add((0.75, 0.25, 1.0), (-tie(5001, 0.125), -tie(5003, 0.125), -tie(6001, 0.125)), -1.0)
    # exactly on nodes: weight 1 at one node, 0 (and -0) at the other seven
    add((_node(3), _node(7), _node(12)), (tie(40000, 1.0), tie(40001, 1.0), -tie(40002, 1.0)))
    add((_node(12), _node(3), _node(5)), (-tie(40003, 1.0), tie(50001, 1.0), tie(50002, 1.0)), 2.0)
    add((_node(8), _node(8), _node(8)), (tie(40004, 1.0), -tie(40005, 1.0), -tie(40006, 1.0)), -1.0)
    # on cell faces (one coordinate on a node plane, the others half-way): weight 1/4 at four nodes
    add((_node(4), 0.5, 0.75), (tie(10000, 0.25), tie(10001, 0.25), -tie(10002, 0.25)))
    add((0.25, _node(9), 1.0), (-tie(10003, 0.25), tie(12000, 0.25), tie(12001, 0.25)), -1.0)
    add((1.125, 0.375, _node(6)), (tie(12002, 0.25), -tie(12003, 0.25), -tie(10005, 0.25)), 2.0)
    # normals at the guard: +-1e4 is an estimate, the next float above is none (the sample votes for nothing, weight included); not finite; tiny; none
    add((0.3, 0.7, 0.9), (1.0e4, -1.0e4, 0.75))
    add((0.31, 0.72, 0.93), (_next_up(1.0e4), 0.5, 0.5))
    add((0.9, 0.2, 0.4), (0.5, -_next_up(1.0e4), 0.5))
    add((0.45, 0.85, 0.15), (np.inf, 0.5, 0.5))
    add((0.46, 0.86, 0.16), (0.5, 0.5, -np.inf), 2.0)
    add((0.47, 0.87, 0.17), (0.5, np.nan, 0.5))
    add((0.6, 0.1, 0.8), (1.0e-40, -1.0e-42, 0.0))
    add((0.61, 0.11, 0.81), (0.0, 0.0, 0.0), -1.0)
    add((_node(10), _node(10), _node(10)), (0.0, -0.0, 0.0))
    # plain rows at general positions, so that the median of the largest components is theirs
    rng = np.random.default_rng(16)
    for r in range(14):
        n = rng.normal(size=3)
        add(tuple(rng.uniform(0.05, 1.2, size=3)), tuple(n / np.abs(n).max() * rng.uniform(0.55, 0.95)), (1.0, 2.0, -1.0)[r % 3])
    return _ro(_rows(np.array(xyz, np.float64), np.array(w))), _ro(np.array(nrm, np.float64).astype(np.float32))


def splat_products(points, normals, G, origin, h):
    """every float32 product n x weight x 2^16 the splat rounds, as splat_kernel forms it (of the samples that vote): for the premise that the
    half-way cases are there.  The normals' scale must be 2^0."""
    p, nrm = np.asarray(points, np.float32), np.asarray(normals, np.float32)
    g = ((p[:, :3] / p[:, 3:4]) - origin[None, :]) / F(h)
    f = np.floor(g)
    ijk = f.astype(np.int64)
    with np.errstate(invalid="ignore"):
        ok = np.all((ijk >= 0) & (ijk + 1 < G), axis=1) & np.all(np.abs(nrm) <= F(1e4), axis=1)
    t = (g - f).astype(np.float32)[ok]
    nrm = nrm[ok]
    out = []
    for c in range(8):
        d = (c & 1, (c >> 1) & 1, c >> 2)
        wgt = (t[:, 0] if d[0] else F(1) - t[:, 0]).astype(np.float32)
        for a in (1, 2):
            wgt = (wgt * (t[:, a] if d[a] else F(1) - t[:, a])).astype(np.float32)
        for ch in range(3):
            out.append(((nrm[:, ch] * wgt).astype(np.float32) * F(65536.0)).astype(np.float32))
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def level_clouds():
    """n -> (xyzw rows, normal rows) for n = 2, 3, 4 samples spanning [0, 1.25]^3: normals of very different lengths, so that chi at the
    samples takes values far apart and the lower median (index (n - 1) // 2 of the sorted values) cannot be mistaken for its neighbours"""
    xyz = np.array([[0.0, 0.0, 0.0], [1.25, 1.25, 1.25], [0.25, 1.0, 0.5], [1.0, 0.25, 0.75]])
    nrm = np.array([[0.9, 0.9, 0.9], [0.0, 0.0, -0.6], [0.5, -0.5, 0.0], [-0.3, 0.0, 0.3]])
    return {n: (_ro(_rows(xyz[:n])), _ro(nrm[:n].astype(np.float32))) for n in (2, 3, 4)}


# ---------------------------------------------------------------------------------------------------------------------------------
# fields for the surface nets: chi[z][y][x] float32, all finite
FIELD_ORIGIN, FIELD_H = np.array([-0.3, 0.1, 2.0], np.float32), F(0.05)
ISO_B = F(0.37)
# the inside / outside pattern of the 9^3 random field, node (k 9 + j) 9 + i = bit (most significant first): found by flipping single nodes
# of a random pattern for as long as that did not lower the number of distinct corner patterns among its 512 cells, until all 254 mixed
# ones were there (a plain random pattern holds about 220 of them)
_SIGNS_G9 = ("1ffc2615998479e1a0449d5f7b36c99d6f21c30a4c691c56d8779f85db9997dbbb92be9910fcb983366c2ad8d93fc3b05381cc357eb1020bcb4c66369c55427a81bec6"
             "24ae18d7b896e9474c88120892dd5b25feda49f719ded15100")


def _grid(G):
    k, j, i = np.meshgrid(np.arange(G), np.arange(G), np.arange(G), indexing="ij")
    return i.astype(np.float64), j.astype(np.float64), k.astype(np.float64)


def _random_field(G, seed):
    rng = np.random.default_rng(seed)
    mag = rng.uniform(0.1, 1.0, size=(G, G, G))
    if G == 9:
        inside = np.unpackbits(np.frombuffer(bytes.fromhex(_SIGNS_G9), np.uint8))[:G ** 3].reshape(G, G, G).astype(bool)
    else:
        inside = rng.integers(0, 2, size=(G, G, G)).astype(bool)
    return np.where(inside, -mag, mag).astype(np.float32)


def corner_cases(chi, iso):
    """the corner pattern of every cell (bit c: corner c inside = chi < iso; corner bits 0 / 1 / 2 = x / y / z) -> int array [z][y][x] of cells"""
    inside = np.asarray(chi, np.float32) < F(iso)
    C = inside.shape[0] - 1
    case = np.zeros((C, C, C), np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
        case |= inside[dz:dz + C, dy:dy + C, dx:dx + C].astype(np.int64) << c
    return case


def _ulps(x, k):
    x = F(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf))
    return x


@functools.lru_cache(maxsize=None)
def fields():
    """name -> dict(chi, iso, origin, h, support (node mask uint8 or None), closed (the level set is a closed surface inside the grid),
    gradient (of a ramp: the direction every face normal must follow, else None), empty (nothing to mesh), two_sided (no edge may have
    more than two facets.  Not so on the random fields: where all four edges of a cell face cross and both cells join the four crossings into
    ONE patch -- a tunnel through the face -- the edge between those two patches carries the four quads of the face's edges; that is the
    method, for the oracle and the kernels alike, and there only the balance of the two directions is asked))"""
    out = {}

    def add(name, chi, iso=0.0, support=None, closed=False, gradient=None, empty=False, both=True, two_sided=True):
        chi = np.asarray(chi, np.float64)
        levels = ((F(0.0), "iso0"), (ISO_B, "iso37")) if both else ((F(iso), None),)
        for level, tag in levels:
            field = (chi + float(level)).astype(np.float32) if both else chi.astype(np.float32)
            assert np.isfinite(field).all()
            out[name + ("-" + tag if tag else "")] = dict(chi=_ro(field), iso=level, origin=FIELD_ORIGIN, h=FIELD_H, support=None if support is None else _ro(support.astype(np.uint8)),
                                                         closed=closed, gradient=gradient, empty=empty, two_sided=two_sided)

    for G in (2, 3, 7, 9, 17):
        add("random-G%d" % G, _random_field(G, 100 + G), two_sided=False)
    i, j, k = _grid(6)
    add("checkerboard-G6", np.where((i + j + k) % 2 == 0, 1.0, -1.0))
    # a slab 0.4 cells thick, inclined to all three axes: |distance to a plane| - 0.2
    i, j, k = _grid(12)
    normal = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    add("slab-G12", np.abs((i - 5.3) * normal[0] + (j - 5.6) * normal[1] + (k - 5.4) * normal[2]) - 0.2)
    i, j, k = _grid(8)
    for axis, coord in enumerate((i, j, k)):
        for sign in (1.0, -1.0):
            grad = np.zeros(3)
            grad[axis] = sign
            add("ramp-%s%s-G8" % ("+" if sign > 0 else "-", "xyz"[axis]), sign * (coord - 3.5) * 0.25, gradient=tuple(grad))
    i, j, k = _grid(12)
    ball = np.sqrt((i - 5.4) ** 2 + (j - 5.7) ** 2 + (k - 5.5) ** 2) - 3.3
    add("sphere-G12", ball, closed=True)
    add("sphere-off-centre-G12", np.sqrt((i - 1.6) ** 2 + (j - 1.3) ** 2 + (k - 1.4) ** 2) - 4.2)
    # masks over the centred sphere: nothing, everything, a half-space that cuts it, one node (the low corner of a mixed cell)
    add("sphere-mask-none-G12", ball, support=np.zeros((12, 12, 12)), empty=True)
    add("sphere-mask-all-G12", ball, support=np.ones((12, 12, 12)), closed=True)
    add("sphere-mask-half-G12", ball, support=(i < 6))
    one = np.zeros((12, 12, 12))
    kk, jj, ii = np.argwhere((corner_cases(ball.astype(np.float32), 0.0) % 255) != 0)[7]
    one[kk, jj, ii] = 1
    add("sphere-mask-one-node-G12", ball, support=one)
    rng = np.random.default_rng(5)
    add("random-mask-random-G7", _random_field(7, 107), support=rng.integers(0, 4, size=(7, 7, 7)) > 0, two_sided=False)
    # nodes equal to the level: "inside" is chi < iso, so they are outside; both kernels must say so
    i, j, k = _grid(7)
    steps = i + 2 * j - k - 3
    for level, tag in ((F(0.0), "iso0"), (ISO_B, "iso37")):
        chi = np.where(steps == 0, np.float64(level), 0.25 * steps + np.float64(level))
        add("nodes-at-the-level-G7-" + tag, chi, iso=level, both=False)
        assert np.count_nonzero(chi.astype(np.float32) == level) > 20
    zero = _random_field(7, 207).astype(np.float64)
    pick = rng.integers(0, 4, size=zero.shape)
    zero[pick == 0] = 0.0
    zero[pick == 1] = -0.0
    add("signed-zeros-G7", zero, iso=0.0, both=False, two_sided=False)
    # nodes one and two float32 steps either side of a level that is itself subnormal: chi - iso is a subnormal of the other sign rule's
    # (cell_flags: chi < iso; cell_vertices: chi - iso < 0): they agree only while subnormals are kept
    tiny = F(1.0e-38)
    near = _random_field(7, 307)
    pick = rng.integers(0, 8, size=near.shape)
    for code, step in ((0, -2), (1, -1), (2, 1), (3, 2)):
        near[pick == code] = _ulps(tiny, step)
    add("nodes-next-to-a-tiny-level-G7", near, iso=tiny, both=False, two_sided=False)
    # nothing to mesh
    add("constant-G5", np.full((5, 5, 5), 0.5), iso=0.0, empty=True, both=False)
    add("constant-at-the-level-G5", np.full((5, 5, 5), 0.37), iso=ISO_B, empty=True, both=False)
    add("below-the-level-G5", -1.0 - 0.1 * _grid(5)[0], iso=0.0, empty=True, both=False)
    return out


def field_names():
    return list(fields().keys())


# ---------------------------------------------------------------------------------------------------------------------------------
# weight fields for the support mask, 16^3 nodes: name -> (weights int64 [z][y][x], R)
MASK_G = 16


@functools.lru_cache(maxsize=None)
def mask_cases():
    out = {}
    G = MASK_G
    for R in (1, 3, 16):
        seeds = {"centre": [(8, 8, 8)], "corner": [(0, 0, 0)], "far-corner": [(15, 15, 15)], "face": [(9, 7, 0)], "none": []}
        if 2 * R + 1 < G - 3:
            seeds["two-seeds"] = [(8, 8, 3), (8, 8, 3 + 2 * R + 1)]       # 2R + 1 apart along x: their masks touch and do not overlap
        for name, nodes in seeds.items():
            w = np.zeros((G, G, G), np.int64)
            w[2, 3, 4] = -5          # only a positive weight is a seed
            for node in nodes:
                w[node] = 1 if name != "face" else 1 << 40
            out["%s-R%d" % (name, R)] = (_ro(w), R)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
def check_mesh(case, v, f, patch_count):
    """what must hold for the surface nets of a field whatever an oracle says (patch_count[256]: the number of patches per corner pattern,
    from the patch table): the counts, every vertex finite and inside the closed cell the grid-order numbering gives it, at most two
    facets per edge (fields()'s two_sided), every edge between vertices of interior cells used as often in one direction as in the other
    (every edge, on a closed surface), faces
    along the gradient of a ramp, and no vertex without a face except in cells on the border of the grid or of the mask"""
    chi, origin, h = case["chi"], case["origin"], F(case["h"])
    v, f = np.asarray(v), np.asarray(f, np.int64).reshape(-1, 3)
    C = chi.shape[0] - 1
    cc = corner_cases(chi, case["iso"])
    cells = np.ones((C, C, C), bool) if case["support"] is None else case["support"][:C, :C, :C].astype(bool)
    per = np.where((cc != 0) & (cc != 255) & cells, np.asarray(patch_count)[cc], 0)
    assert len(v) == per.sum() and v.shape == (len(v), 4) and v.dtype == np.float32
    if case["empty"]:
        assert len(v) == 0 and len(f) == 0
        return
    assert len(v) > 0 and len(f) % 2 == 0
    assert np.isfinite(v).all() and np.all(v[:, 3] == 1.0)
    cell = np.repeat(np.arange(C ** 3), per.ravel())
    ijk = np.stack([cell % C, cell // C % C, cell // (C * C)], 1)
    for axis in range(3):     # the kernel's own operations on the cell's two faces: rounding is monotone, so the bounds are exact
        lo = (origin[axis] + (h * ijk[:, axis].astype(np.float32)).astype(np.float32)).astype(np.float32)
        hi = (origin[axis] + (h * (ijk[:, axis] + 1).astype(np.float32)).astype(np.float32)).astype(np.float32)
        assert np.all((lo <= v[:, axis]) & (v[:, axis] <= hi)), axis
    if len(f) == 0:
        used = np.zeros(len(v), bool)
    else:
        assert f.min() >= 0 and f.max() < len(v)
        assert np.all(f[:, 0] != f[:, 1]) and np.all(f[:, 1] != f[:, 2]) and np.all(f[:, 2] != f[:, 0])
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        und = np.sort(e, 1)
        facets = np.unique(und[:, 0] * len(v) + und[:, 1], return_counts=True)[1]
        assert facets.max() <= (2 if case["two_sided"] else 4)
        used = np.zeros(len(v), bool)
        used[f.ravel()] = True
    # interior: the cell and its 26 neighbours exist and are meshed
    pad = np.zeros((C + 2, C + 2, C + 2), bool)
    pad[1:-1, 1:-1, 1:-1] = cells
    inner = np.ones((C, C, C), bool)
    for dk in range(3):
        for dj in range(3):
            for di in range(3):
                inner &= pad[dk:dk + C, dj:dj + C, di:di + C]
    interior = inner.ravel()[cell]
    assert used[interior].all()
    if case["closed"]:
        assert used.all() and (case["support"] is not None or interior.all())
    if len(f):
        fwd = dict(zip(*np.unique(e[:, 0] * len(v) + e[:, 1], return_counts=True)))
        for (a, b) in e[(interior[e[:, 0]] & interior[e[:, 1]]) | case["closed"]].tolist():
            assert fwd[a * len(v) + b] == fwd.get(b * len(v) + a, 0) <= (1 if case["two_sided"] else 2), (a, b)
    if case["gradient"] is not None:
        p = v[:, :3].astype(np.float64)[f]
        normal = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        assert len(f) and np.all(normal @ np.array(case["gradient"]) > 0.0)
