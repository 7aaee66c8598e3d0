"""numpy restatement of the windowed matching cost, written from the contract and not from the kernel.  It is the
arbiter: mvs_sweep_window must be bit-identical to window().

Integers only (int64: the largest product, S n with S below 2^31 and n below 2^9, stays below 2^40).  Volumes are [D, H, W] uint32 packed
cells count << cs | sum; `cs` is 24 for the fixed sampler and 16 for the exact one; the guide is [H, W] uint8."""
import numpy as np


def split(vol, cs):
    """packed cells -> (sum, count) as int64"""
    v = np.asarray(vol, np.uint32).astype(np.int64)
    return v & ((1 << cs) - 1), v >> cs


def window(vol, cs, radius, tau=255, guide=None):
    """Wv: for every pixel p and plane d, n(p, d) << cs | floor(S n(p, d) / N) with S, N the sums of the cost sums and counts of the seen
    cells q of the frame with |q.row - p.row| <= radius, |q.col - p.col| <= radius and |G(q) - G(p)| <= tau; 0 where n(p, d) = 0"""
    assert 0 <= radius <= 4 and 0 <= tau <= 255
    s, n = split(vol, cs)
    s = np.where(n > 0, s, 0)          # a member no view sees adds nothing, whatever its sum field holds
    D, H, W = s.shape
    S, N = np.zeros_like(s), np.zeros_like(n)
    G = None if tau == 255 else np.asarray(guide, np.uint8).astype(np.int64)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)    # the pixels p whose neighbour p + (dy, dx) is in the frame
            if y0 >= y1 or x0 >= x1:
                continue
            p, q = (slice(None), slice(y0, y1), slice(x0, x1)), (slice(None), slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
            member = 1 if G is None else (np.abs(G[q[1:]] - G[p[1:]]) <= tau)[None]
            S[p] += s[q] * member
            N[p] += n[q] * member
    quotient = np.where(n > 0, (S * n) // np.maximum(N, 1), 0)
    assert quotient.max() < (1 << cs), "the volume breaks the contract's premise (a sum above count * the largest per-sample cost)"
    return np.where(n > 0, (n << cs) | quotient, 0).astype(np.uint32)
