"""Exact-arithmetic specification check of the oracle's GEOS slice (the ring cull of a-8).

shapely / GEOS cannot be obtained in this image, so these functions have no reference-generated vector ("parity
unpinned").  What CAN be checked is GEOS's *contract*: `LinearRing.intersects` is decided by
RobustLineIntersector, whose only inexact ingredient -- `Orientation::index` -- is defined to return the EXACT sign of
the orientation determinant (CGAlgorithmsDD falls back to extended precision).  So "do two closed segments with these
double coordinates share a point" has one right answer, computable with `fractions.Fraction` on the exact binary
values of the inputs.  This file compares the oracle with that answer on > 10^5 adversarial cases (collinear overlaps,
touching endpoints, T-junctions, 1-ulp perturbations of all of them, DLP-sized coordinate offsets), and bounds the
continuous functions (convex-quad overlap area, point-segment distance) against exact rational evaluation.
"""
import math

import numpy as np
import pytest

from exact_geometry import (F, OFFSETS, adversarial_segments, clip_area_exact, orient_exact, orientation_triples,
                            point_segment_cases, pt_seg_dist2_exact, quad_pairs, seg_intersect_exact)
from oracle import oracle as O


@pytest.mark.parametrize('seed', [0, 1])
def test_segments_intersect_is_the_exact_predicate(seed):
    """a-3: 2 x ~87k adversarial pairs, oracle == exact rational answer on every one."""
    rng = np.random.default_rng(seed)
    n = hits = 0
    kinds = {True: 0, False: 0}
    for p1, p2, q1, q2 in adversarial_segments(rng, 50000):
        want = seg_intersect_exact(p1, p2, q1, q2)
        got = O.segments_intersect(p1, p2, q1, q2)
        assert got == want, (p1, p2, q1, q2, got, want)
        kinds[want] += 1
        n += 1
    assert n > 80000 and min(kinds.values()) > 15000           # both answers well represented


def test_orientation_is_the_exact_sign():
    rng = np.random.default_rng(5)
    zero = 0
    for a, b, c in orientation_triples(rng, 40000):
        want = orient_exact(F(a), F(b), F(c))
        assert O.orient(a, b, c) == want
        zero += want == 0
    assert zero > 10000


def test_ring_intersects_boundary_semantics_exact():
    """LinearRing.intersects(LinearRing): boundaries only -- any edge pair shares a point; containment is False."""
    rng = np.random.default_rng(2)
    from hope_amd.scenes import create_box
    n_true = n_false = 0
    for k in range(6000):
        ox, oy = OFFSETS[k % 3]
        hull = create_box((ox + rng.uniform(-2, 2), oy + rng.uniform(-2, 2), rng.uniform(-4, 4)))
        nv = 3 if k % 5 == 0 else 4
        if k % 4 == 0:                                          # big ring around the hull (containment) or far away
            c = np.array([ox, oy]) + (0 if k % 8 == 0 else 40)
            ring = c + np.array([[-12, -12], [12, -12], [12, 12], [-12, 12]], float)[:nv]
        elif k % 4 == 1:                                        # ring sharing exactly one hull corner
            ring = hull[int(rng.integers(4))] + np.vstack([[0, 0], rng.uniform(-3, 3, (nv - 1, 2))])
        else:
            ang = rng.uniform(0, 2 * np.pi)
            r = rng.uniform(0.3, 2.5)
            c = np.array([ox, oy]) + rng.uniform(-5, 5, 2)
            ring = c + r * np.column_stack([np.cos(ang + np.arange(nv) * 2 * np.pi / nv), np.sin(ang + np.arange(nv) * 2 * np.pi / nv)])
        want = any(seg_intersect_exact(hull[i], hull[(i + 1) % 4], ring[j], ring[(j + 1) % nv])
                   for i in range(4) for j in range(nv))
        assert O.ring_intersects(hull, ring) == want, k
        n_true += want
        n_false += not want
    assert n_true > 1500 and n_false > 1500


# ---- continuous functions: bounded against exact rational evaluation ----------------------------------------------------
def test_quad_overlap_area_against_exact_rational():
    """a-4 / box-union term of a-12: |hull ∩ dest| for two car-sized rectangles.  The oracle's float64 clip must agree
    with the exact area to 1e-12 m^2 (area ~ 9.1 m^2), and the `> 0.95` arrival decision may only differ from the exact
    one inside that band."""
    from hope_amd.scenes import create_box
    rng = np.random.default_rng(3)
    worst, close = 0.0, 0
    for k, (A, B) in enumerate(quad_pairs(rng, 3000)):
        exact = clip_area_exact(A, B)
        got = O.quad_intersection_area(A, B)
        err = abs(got - float(exact))
        worst = max(worst, err)
        area_b = O.quad_area(B)
        ratio_exact = float(exact) / area_b
        if abs(ratio_exact - 0.95) > 1e-12:
            assert (got / area_b > 0.95) == (ratio_exact > 0.95), k
        close += abs(ratio_exact - 0.95) < 0.02
    assert worst < 1e-12, worst
    assert close > 100
    # closed forms: identical boxes -> the box area; disjoint -> 0; half overlap along the axis
    B = create_box((3.0, -2.0, 0.0))
    assert abs(O.quad_intersection_area(B, B) - 4.69 * 1.94) < 1e-13 and abs(O.quad_area(B) - 4.69 * 1.94) < 1e-13
    assert O.quad_intersection_area(create_box((40.0, 0.0, 0.3)), B) == 0.0
    assert abs(O.quad_intersection_area(create_box((3.0 + 4.69 / 2, -2.0, 0.0)), B) - 4.69 * 1.94 / 2) < 1e-13


def test_point_segment_distance_against_exact_rational():
    """ring cull of a-8 (`LinearRing.distance(Point) < 10`): Distance::pointToSegment to a few ulp of the exact value,
    so the keep/drop decision can only differ from the exact one within ~1e-14 m of the 10 m boundary."""
    rng = np.random.default_rng(4)
    worst = 0.0
    for k, (p, a, b) in enumerate(point_segment_cases(rng, 20000)):
        d2 = pt_seg_dist2_exact(p, a, b)
        want = math.sqrt(float(d2))
        got = O.pt_seg_dist(p, a, b)
        rel = abs(got - want) / max(want, 1e-300)
        worst = max(worst, rel)
        if abs(want - 10.0) > 1e-13:
            assert (got < 10.0) == (d2 < 100), k
    assert worst < 2e-14, worst          # perpendicular foot near an endpoint of a ~20 m lever arm: a handful of ulps
