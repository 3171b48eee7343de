"""Exact predicates on the binary values of float64 inputs (`fractions.Fraction`), the adversarial case generators built on
them, and a numpy mirror of the device's orientation FILTER.  Shared by tests/test_oracle_exact_geometry.py (the CPU oracle
against exact arithmetic), tests/test_gpu_exact_geometry.py (the device's exact path against both) and tests/touching_scenes.py.
The generators draw from the caller's `rng` in a fixed order: the same seed gives the same cases in every file."""
import math
from fractions import Fraction as Fr

import numpy as np

OFFSETS = [(0.0, 0.0), (147.25, -36.5), (-83.0, 61.125), (1e4, 1e4)]
UNDECIDED = 2               # ORIENT_UNDECIDED / segments_intersect_fast's "undecided" (hope_amd/csrc/hope_dev.h)


# ---- exact predicates on the binary values of the inputs -------------------------------------------------------------
def F(p):
    return (Fr(float(p[0])), Fr(float(p[1])))


def orient_exact(a, b, c):
    d = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
    return (d > 0) - (d < 0)


def on_seg(a, b, c):
    """c collinear with ab: inside the closed segment?"""
    return min(a[0], b[0]) <= c[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= c[1] <= max(a[1], b[1])


def seg_intersect_exact(p1, p2, q1, q2):
    p1, p2, q1, q2 = F(p1), F(p2), F(q1), F(q2)
    o1, o2 = orient_exact(p1, p2, q1), orient_exact(p1, p2, q2)
    o3, o4 = orient_exact(q1, q2, p1), orient_exact(q1, q2, p2)
    if o1 * o2 < 0 and o3 * o4 < 0:
        return True
    return ((o1 == 0 and on_seg(p1, p2, q1)) or (o2 == 0 and on_seg(p1, p2, q2)) or
            (o3 == 0 and on_seg(q1, q2, p1)) or (o4 == 0 and on_seg(q1, q2, p2)))


def boxes_apart(p1, p2, q1, q2):
    """the coordinate boxes of the two segments are disjoint (comparisons of doubles are exact): no common point"""
    return (min(p1[0], p2[0]) > max(q1[0], q2[0]) or max(p1[0], p2[0]) < min(q1[0], q2[0]) or
            min(p1[1], p2[1]) > max(q1[1], q2[1]) or max(p1[1], p2[1]) < min(q1[1], q2[1]))


def hull_edge_intersect_exact(box, q1, q2):
    """any of the four edges of the hull `box` [4][2] shares a point with the closed segment q1 q2"""
    return any(not boxes_apart(box[k], box[(k + 1) % 4], q1, q2) and seg_intersect_exact(box[k], box[(k + 1) % 4], q1, q2)
               for k in range(4))


def collision_exact(box, quads):
    """_detect_collision on exact arithmetic: any hull edge x any edge of any quad [m][4][2]"""
    return any(hull_edge_intersect_exact(box, q[j], q[(j + 1) % 4]) for q in quads for j in range(4))


def ulp_nudge(rng, pts):
    """move one random coordinate of one random point by +-1..2 ulp"""
    pts = [list(p) for p in pts]
    i, j = int(rng.integers(len(pts))), int(rng.integers(2))
    for _ in range(int(rng.integers(1, 3))):
        pts[i][j] = float(np.nextafter(pts[i][j], math.inf if rng.random() < 0.5 else -math.inf))
    return [tuple(p) for p in pts]


def dyadic(rng, lo, hi, bits=10):
    """a double that is an exact multiple of 2^-bits (sums / differences of a few of them are exact)"""
    return float(rng.integers(int(lo * 2 ** bits), int(hi * 2 ** bits))) / 2 ** bits


def adversarial_segments(rng, n):
    """yields (p1, p2, q1, q2) tuples"""
    for k in range(n):
        ox, oy = OFFSETS[k % len(OFFSETS)]
        kind = k % 8
        if kind == 0:                                       # generic random pair in a 6 m window
            pts = [(ox + rng.uniform(-3, 3), oy + rng.uniform(-3, 3)) for _ in range(4)]
        elif kind in (1, 2):                                # exactly collinear (dyadic direction x small integers)
            bx, by, dx, dy = dyadic(rng, -3, 3), dyadic(rng, -3, 3), dyadic(rng, -1, 1), dyadic(rng, -1, 1)
            ts = rng.integers(-6, 7, 4)
            pts = [(ox + bx + int(t) * dx, oy + by + int(t) * dy) for t in ts]
            if ox == 1e4:
                pts = [(bx + int(t) * dx, by + int(t) * dy) for t in ts]      # keep the sums exact
        elif kind == 3:                                     # shared endpoint
            pts = [(ox + rng.uniform(-3, 3), oy + rng.uniform(-3, 3)) for _ in range(3)]
            pts = [pts[0], pts[1], pts[1], pts[2]] if rng.random() < 0.5 else [pts[0], pts[1], pts[2], pts[0]]
        elif kind == 4:                                     # T-junction: q1 exactly the midpoint of a dyadic p
            a = (dyadic(rng, -3, 3, 8), dyadic(rng, -3, 3, 8))
            d = (dyadic(rng, -2, 2, 8), dyadic(rng, -2, 2, 8))
            p1, p2 = a, (a[0] + 2 * d[0], a[1] + 2 * d[1])
            mid = (a[0] + d[0], a[1] + d[1])
            pts = [p1, p2, mid, (mid[0] + rng.uniform(-2, 2), mid[1] + rng.uniform(-2, 2))]
        elif kind == 5:                                     # axis-aligned walls (the DLP lots are full of them)
            x = dyadic(rng, -3, 3)
            pts = [(ox + x, oy + rng.uniform(-3, 3)), (ox + x, oy + rng.uniform(-3, 3)),
                   (ox + rng.uniform(-3, 3), oy + dyadic(rng, -3, 3)), (ox + rng.uniform(-3, 3), oy + dyadic(rng, -3, 3))]
            if rng.random() < 0.5:
                pts[2] = (ox + x, pts[2][1])                # endpoint exactly on the wall's line
        elif kind == 6:                                     # nearly parallel, nearly touching
            a = np.array([ox + rng.uniform(-3, 3), oy + rng.uniform(-3, 3)])
            d = rng.normal(size=2)
            e = d * (1 + 1e-13 * rng.normal()) + 1e-13 * rng.normal(size=2)
            pts = [tuple(a), tuple(a + d), tuple(a + 0.5 * d + 1e-14 * rng.normal(size=2)), tuple(a + 0.5 * d + e)]
        else:                                               # a vertex of one segment 1e-16-close to the other's line
            a = np.array([ox + rng.uniform(-3, 3), oy + rng.uniform(-3, 3)])
            d = rng.normal(size=2)
            t = rng.uniform(-0.2, 1.2)
            pts = [tuple(a), tuple(a + d), tuple(a + t * d), tuple(a + t * d + rng.normal(size=2))]
        yield tuple(pts)
        if kind in (1, 2, 3, 4, 5, 7):
            yield tuple(ulp_nudge(rng, pts))


def touching_segments(rng, n):
    """More of adversarial_segments' kinds 4 and 7, always with the ulp nudge / inside the other segment and mostly at coordinates of
    a few metres, where one ulp lies inside the filter's error band: pairs that the orientation filter leaves open and whose
    exact answer is "no common point" nearly as often as "a common point" (in adversarial_segments kind 7 always sits at the 1e4
    offset, where the filter decides it).  yields (p1, p2, q1, q2)"""
    for k in range(n):
        ox, oy = OFFSETS[1 + (k // 16) % 2] if k % 16 < 2 else OFFSETS[0]
        if k % 2 == 0:                                      # T-junction on dyadic coordinates, one coordinate moved by 1-2 ulp
            a = (ox + dyadic(rng, -3, 3, 8), oy + dyadic(rng, -3, 3, 8))
            d = (dyadic(rng, -2, 2, 8), dyadic(rng, -2, 2, 8))
            mid = (a[0] + d[0], a[1] + d[1])
            pts = [a, (a[0] + 2 * d[0], a[1] + 2 * d[1]), mid, (mid[0] + rng.uniform(-2, 2), mid[1] + rng.uniform(-2, 2))]
            yield tuple(ulp_nudge(rng, pts))
        else:                                               # q1 on p up to the rounding of a + t d
            a = np.array([ox + rng.uniform(-3, 3), oy + rng.uniform(-3, 3)])
            d = rng.normal(size=2)
            t = rng.uniform(0.05, 0.95)
            yield tuple(a), tuple(a + d), tuple(a + t * d), tuple(a + t * d + rng.normal(size=2))


def orientation_triples(rng, n=40000):
    """yields (a, b, c): c on the line ab up to rounding, every third triple exactly collinear and dyadic"""
    for k in range(n):
        ox, oy = OFFSETS[k % len(OFFSETS)]
        a = np.array([ox + rng.uniform(-3, 3), oy + rng.uniform(-3, 3)])
        d = rng.normal(size=2)
        t = rng.uniform(-1, 2)
        c = a + t * d                                           # on the line up to rounding: the filter must give way
        if k % 3 == 0:                                          # exactly collinear dyadic triple
            a = np.array([dyadic(rng, -3, 3), dyadic(rng, -3, 3)])
            d = np.array([dyadic(rng, -1, 1), dyadic(rng, -1, 1)])
            c = a + 3 * d
        b = a + d
        yield a, b, c


def quad_pairs(rng, n=3000):
    """yields (A, B) = (hull of an ego pose, box of a dest pose): near-arrival, generic and same-heading pairs in turn"""
    from hope_amd.scenes import create_box
    for k in range(n):
        ox, oy = OFFSETS[k % 3]
        dest = (ox + rng.uniform(-2, 2), oy + rng.uniform(-2, 2), rng.uniform(-4, 4))
        if k % 3 == 0:                                           # near-arrival poses: ratios around 0.95
            ego = (dest[0] + rng.normal() * 0.06, dest[1] + rng.normal() * 0.06, dest[2] + rng.normal() * 0.01)
        elif k % 3 == 1:
            ego = (dest[0] + rng.uniform(-5, 5), dest[1] + rng.uniform(-3, 3), dest[2] + rng.uniform(-1, 1))
        else:                                                    # same heading, pure translation (parallel edges)
            ego = (dest[0] + rng.uniform(-5, 5), dest[1] + rng.uniform(-2, 2), dest[2])
        yield create_box(ego), create_box(dest)


def degenerate_quad_pairs(rng, n):
    """yields (A, B), convex CCW quads in the positions a Sutherland-Hodgman clip has to get right without room for rounding: B = A
    bit for bit; A moved along one of its own edges by a dyadic amount (shared collinear edges), on dyadic and on rotated
    coordinates; a vertex of A exactly on an edge of B, from outside and from inside; A inside B; disjoint"""
    from hope_amd.scenes import create_box
    for k in range(n):
        ox, oy = OFFSETS[k % 3]
        x0, y0, w, h = ox + dyadic(rng, -3, 3), oy + dyadic(rng, -3, 3), dyadic(rng, 1, 5), dyadic(rng, 1, 3)
        R = np.array([[x0, y0], [x0 + w, y0], [x0 + w, y0 + h], [x0, y0 + h]])          # dyadic, axis-aligned
        H = create_box((ox + rng.uniform(-2, 2), oy + rng.uniform(-2, 2), rng.uniform(-4, 4)))
        kind = k % 8
        if kind == 0:
            yield H, H.copy()
        elif kind == 1:
            yield R, R + np.array([dyadic(rng, -6, 6), 0.0])
        elif kind == 2:                                          # along a rotated hull's own edge: collinear up to rounding
            j = int(rng.integers(4))
            yield H, H + dyadic(rng, -1, 1, 4) * (H[(j + 1) % 4] - H[j])
        elif kind in (3, 4):                                     # a diamond with its lowest vertex on R's top (3) or bottom (4) edge
            s = dyadic(rng, 0, 1, 6) + 2.0 ** -6
            v = np.array([x0 + dyadic(rng, 0, 1, 8) * w, y0 + (h if kind == 3 else 0.0)])
            yield v + np.array([[0, 0], [s, s], [0, 2 * s], [-s, s]]), R
        elif kind == 5:                                          # A inside B
            c = R.mean(axis=0)
            yield c + 0.25 * (R - c), R
        elif kind == 6:                                          # B inside A, rotated
            c = H.mean(axis=0)
            yield H, c + rng.uniform(0.1, 0.9) * (H - c)
        else:
            yield H, H + np.array([rng.uniform(6, 9), rng.uniform(-9, 9)])


def point_segment_cases(rng, n=20000):
    """yields (p, a, b): a point and a segment within ~14 m of it, every tenth segment degenerate"""
    for k in range(n):
        ox, oy = OFFSETS[k % 3]
        p = (ox + rng.uniform(-1, 1), oy + rng.uniform(-1, 1))
        a = (p[0] + rng.uniform(-14, 14), p[1] + rng.uniform(-14, 14))
        b = (a[0] + rng.uniform(-6, 6), a[1] + rng.uniform(-6, 6)) if k % 10 else a          # degenerate segment too
        yield p, a, b


# ---- continuous functions on exact rationals ------------------------------------------------------------------------
def clip_area_exact(A, B):
    """Sutherland-Hodgman of convex CCW quad A by the half-planes of convex CCW quad B, shoelace, all in Fraction."""
    poly = [F(p) for p in A]
    Bq = [F(p) for p in B]
    for e in range(4):
        c1, c2 = Bq[e], Bq[(e + 1) % 4]
        ex, ey = c2[0] - c1[0], c2[1] - c1[1]
        out = []
        for i in range(len(poly)):
            s, t = poly[i], poly[(i + 1) % len(poly)]
            ds = ex * (s[1] - c1[1]) - ey * (s[0] - c1[0])
            dt = ex * (t[1] - c1[1]) - ey * (t[0] - c1[0])
            if ds >= 0:
                out.append(s)
            if (ds >= 0) != (dt >= 0):
                r = ds / (ds - dt)
                out.append((s[0] + r * (t[0] - s[0]), s[1] + r * (t[1] - s[1])))
        poly = out
        if not poly:
            return Fr(0)
    a = sum(poly[i][0] * poly[(i + 1) % len(poly)][1] - poly[(i + 1) % len(poly)][0] * poly[i][1] for i in range(len(poly)))
    return abs(a) / 2


def pt_seg_dist2_exact(p, a, b):
    """the exact SQUARE of the distance from p to the closed segment ab"""
    P, A, B = F(p), F(a), F(b)
    dx, dy = B[0] - A[0], B[1] - A[1]
    l2 = dx * dx + dy * dy
    if l2 == 0:
        return (P[0] - A[0]) ** 2 + (P[1] - A[1]) ** 2
    r = ((P[0] - A[0]) * dx + (P[1] - A[1]) * dy) / l2
    r = min(max(r, Fr(0)), Fr(1))
    cx, cy = A[0] + r * dx, A[1] + r * dy
    return (P[0] - cx) ** 2 + (P[1] - cy) ** 2


# ---- numpy mirror of the device's orientation filter (hope_amd/csrc/hope_dev.h; numpy does not contract a * b - c) ---------
def orient_filter_np(ax, ay, bx, by, cx, cy):
    """orient_filter on arrays: the sign where the filter decides, UNDECIDED elsewhere"""
    ax, ay, bx, by, cx, cy = (np.asarray(v, np.float64) for v in (ax, ay, bx, by, cx, cy))
    dl = (ax - cx) * (by - cy)
    dr = (ay - cy) * (bx - cx)
    det = dl - dr
    sg = np.sign(det).astype(np.int32)
    opposite = ((dl > 0) & (dr <= 0)) | ((dl < 0) & (dr >= 0)) | (dl == 0)
    detsum = np.where(dl > 0, dl + dr, -dl - dr)
    err = 1e-15 * detsum
    decided = opposite | (det >= err) | (-det >= err)
    return np.where(decided, sg, UNDECIDED).astype(np.int32)


def segments_fast_np(p1x, p1y, p2x, p2y, q1x, q1y, q2x, q2y):
    """segments_intersect_fast on arrays: 0 no common point, 1 a common point, UNDECIDED"""
    a = [np.asarray(v, np.float64) for v in (p1x, p1y, p2x, p2y, q1x, q1y, q2x, q2y)]
    p1x, p1y, p2x, p2y, q1x, q1y, q2x, q2y = np.broadcast_arrays(*a)
    apart = (np.minimum(p1x, p2x) > np.maximum(q1x, q2x)) | (np.maximum(p1x, p2x) < np.minimum(q1x, q2x)) | \
            (np.minimum(p1y, p2y) > np.maximum(q1y, q2y)) | (np.maximum(p1y, p2y) < np.minimum(q1y, q2y))
    Pq1 = orient_filter_np(p1x, p1y, p2x, p2y, q1x, q1y)
    Pq2 = orient_filter_np(p1x, p1y, p2x, p2y, q2x, q2y)
    Qp1 = orient_filter_np(q1x, q1y, q2x, q2y, p1x, p1y)
    Qp2 = orient_filter_np(q1x, q1y, q2x, q2y, p2x, p2y)
    same = lambda u, v: ((u == 1) & (v == 1)) | ((u == -1) & (v == -1))
    miss = apart | same(Pq1, Pq2) | same(Qp1, Qp2)
    und = (Pq1 == UNDECIDED) | (Pq2 == UNDECIDED) | (Qp1 == UNDECIDED) | (Qp2 == UNDECIDED)
    return np.where(miss, 0, np.where(und, UNDECIDED, 1)).astype(np.int32)


def collision_fast_np(box, quads):
    """The filter's view of detect_collision for hulls box [..., 4, 2] against quads [..., m, 4, 2] (leading axes broadcast):
    (certain, open) -- `certain`: some (hull edge, obstacle edge) pair is a hit the filter is sure of; `open`: number of obstacle
    edges with a pair the filter leaves undecided.  The robust path runs where open > 0 and not certain."""
    quads = np.asarray(quads, np.float64)
    b1 = np.asarray(box, np.float64)[..., None, None, :, :]               # [..., 1(m), 1(j), 4(k), 2]
    b2 = np.roll(b1, -1, axis=-2)
    q1 = quads[..., :, :, None, :]                                        # [..., m, 4(j), 1, 2]
    q2 = np.roll(quads, -1, axis=-2)[..., :, :, None, :]
    r = segments_fast_np(b1[..., 0], b1[..., 1], b2[..., 0], b2[..., 1], q1[..., 0], q1[..., 1], q2[..., 0], q2[..., 1])
    certain = (r == 1).any(axis=(-1, -2, -3))
    open_ = (r == UNDECIDED).any(axis=-1).sum(axis=(-1, -2))
    return certain, open_
