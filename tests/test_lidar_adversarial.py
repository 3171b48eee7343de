"""The premise of tests/test_gpu_lidar_adversarial.py, checked without a GPU, and an anchor for the oracle's lidar that does not
go through the reference's golden vectors.

Premise: the lots of tests/lidar_adversarial.py reach the filter branches they are aimed at.  The branch predicates of the lidar
stage (hope_amd/csrc/hope_step_kernel.h, hope_amd/csrc/hope_obs_pair.h) are restated in numpy by lidar_adversarial.census; every
branch has to be populated by at least MIN_BRANCH lots, every listed offset of a straddled threshold by MIN_SIDE lots on each
side.  Where the target is the threshold itself (1e-9 m off a beam's line, ring distance 10 (1 +- 5e-10)) only the number of lots
is asserted, not the side they land on.

Anchor: on the generic family the oracle's range per beam is compared with the exact nearest hit (fractions.Fraction on the
binary values of the ego coordinates and of the beam table); on families 1-3 the decisions that exact arithmetic fixes -- a ring
at an exact distance >= 10 gives no hit, a ring clearly nearer that a clean beam crosses gives one -- are asserted ring by ring."""
import collections
import functools
import math

import numpy as np

import lidar_adversarial as A

MIN_BRANCH, MIN_SIDE = 8, 4


@functools.lru_cache(maxsize=None)
def table():
    """(lot, census) of every lot of lidar_adversarial.all_lots"""
    return [(l, A.census(l)) for l in A.all_lots()]


def _sel(fam, *tag):
    return [(l, c) for l, c in table() if l.fam == fam and l.tag[:len(tag)] == tag]


def _sides(fam, kind, offsets, n_min=MIN_SIDE):
    """every offset has >= n_min lots on each side (the offset 0 has one side) -> {(offset, side): lots}"""
    out = {}
    for off in offsets:
        for sgn in ((1,) if off == 0 else (1, -1)):
            rows = [(l, c) for l, c in _sel(fam, kind, off) if l.tag[2] == sgn]
            assert len(rows) >= n_min, (fam, kind, off, sgn, len(rows))
            out[(off, sgn)] = rows
    return out


def test_family_1_beam_aligned_lots_reach_near_beam_thin_and_the_line_test():
    """Counts (lots): vertex on a beam 56 at offset 0, 64 on each side of 1e-5, 2e-4 and 3e-4 rad: near_beam holds for every
    lot up to 2e-4 and for none at 3e-4 (whose ring is culled); edge on an axis beam's line 16 at 0 and 16 on each side of 1e-10,
    1e-9 and 1e-8 m: (beam, edge) pairs with both end points within beam_may_hit's 1e-9 in every lot below 1e-9, in none at 1e-8;
    front edge of extent 0 / 5e-5 m thin in all 6 + 12 lots, of 2e-4 m in none of 12; an end point with y = 0 on the -x axis in
    12 lots, on the +x axis in 12; of the 6 + 6 written as y = -0.0 in the world, all 6 on the +x axis reach the ego frame as -0.0
    (the beam 0 / 119 wrap of the span) and none on the -x axis: at heading 0 the transform adds (+0.0) to it there, at any other
    heading an exact cancellation rounds to +0.0, so no pose can deliver one (tests/lidar_adversarial.py, family_beam_aligned)."""
    v = _sides(1, 'vertex', A.OFF_BEAM)
    for (off, sgn), rows in v.items():
        for l, c in rows:
            f = c['first']
            assert f['kept'] and not f['wild'], l.tag
            if off <= 2e-4:
                assert f['near_beam'] and not f['culled'], (l.tag, l.pose)
            else:
                assert not f['near_beam'] and f['culled'], (l.tag, l.pose)
    assert sum(len(r) for (off, s), r in v.items() if off <= 2e-4) >= MIN_BRANCH and sum(len(r) for (off, s), r in v.items() if off > 2e-4) >= MIN_BRANCH
    col = _sides(1, 'collinear', A.OFF_COLLINEAR)
    for (off, sgn), rows in col.items():
        for l, c in rows:
            if off < 1e-9:
                assert c['first']['on_line_pairs'] >= 1, l.tag
            elif off > 1e-9:
                assert c['first']['on_line_pairs'] == 0, l.tag
    assert sum(c['det0'] > 0 for l, c in _sel(1, 'collinear', 0.0)) >= MIN_BRANCH         # det == 0: the reference's "parallel"
    th = _sides(1, 'thin', A.OFF_THIN)
    for (ext, sgn), rows in th.items():
        for l, c in rows:
            assert c['first']['thin'] == (ext < 1e-4) and c['first']['both_facings'], l.tag
    assert sum(len(r) for (e, s), r in th.items() if e < 1e-4) >= MIN_BRANCH and sum(len(r) for (e, s), r in th.items() if e > 1e-4) >= MIN_BRANCH
    for axis in ('neg_x', 'pos_x'):
        rows = _sel(1, 'zero_y', axis)
        assert len(rows) >= MIN_BRANCH and all(c['first']['zero_y_' + axis] >= 1 for l, c in rows), axis
    minus = {axis: [c['first']['zero_y_minus'] for l, c in _sel(1, 'zero_y', axis, 'minus')] for axis in ('neg_x', 'pos_x')}
    assert len(minus['pos_x']) >= MIN_SIDE and all(m >= 1 for m in minus['pos_x']), minus      # y = -0.0 reaches the oracle and the device
    assert len(minus['neg_x']) >= MIN_SIDE and not any(minus['neg_x']), minus                  # (cannot: see the docstring)
    assert not any(c['first']['zero_y_minus'] for l, c in _sel(1, 'zero_y') if l.tag[2] == 'plus')
    print('family 1:', {k: len(r) for k, r in v.items()}, {k: len(r) for k, r in col.items()}, {k: len(r) for k, r in th.items()},
          'y = -0.0 end points:', sum(c['first']['zero_y_minus'] for l, c in _sel(1, 'zero_y')))


def test_family_2_range_ties_reach_the_ring_fallback_and_the_near_list_slack():
    """Counts (lots): three rings (an edge at x = 10, a vertex at (6, 8), a foot inside an edge) x four quarter turns x exact and
    rounded pose: 24 at distance exactly 10, 24 on each side of 10 (1 +- k 1e-10), k = 1, 5, 20, and 12 + 12 well inside / outside.
    The squared-quantity test leaves 95 rings to the exact fallback (every lot at 10 and at k = 1), keeps 56 and drops 41 outright;
    10 rings whose COMPUTED distance is exactly 10.0 (dropped) while a beam's computed hit on them is below 10 (`<=` for `<` in the
    ring test shows in the scan); boxes at 10 m + 1e-5 miss the near list (8 lots), at 10 m + 1e-7 are listed and dropped (8), at
    10 m - 1e-7 / 1e-5 kept (16); 12 lots with a hit at exactly 10 m, 24 with hits beyond."""
    rows = _sel(2, 'ring')
    tally = collections.Counter()
    for l, c in rows:
        f = c['first']
        name, k, sgn = l.tag[1:]
        tally[(k, sgn)] += 1
        tally['amb' if f['amb'] else 'keep' if f['keep_decided'] else 'drop'] += 1
        if k in (0, 1):
            assert f['amb'], (l.tag, l.pose)                        # inside the margin: the exact path decides
        if k == 'well':
            assert not f['amb'] and f['kept'] == (sgn < 0), l.tag
    for k in A.OFF_RING:
        assert tally[(k, 1)] >= MIN_SIDE and tally[(k, -1)] >= MIN_SIDE, (k, tally)
    assert tally[(0, 0)] >= MIN_BRANCH and min(tally['amb'], tally['keep'], tally['drop']) >= MIN_BRANCH, tally
    comp = _sel(2, 'tie', 'computed_10')                                 # dropped at a COMPUTED distance of exactly 10.0, yet a hit below 10 if kept
    assert len(comp) >= MIN_BRANCH
    for l, c in comp:
        assert np.array_equal(l.ego(), l.quads) and c['first']['amb'] and not c['first']['kept'], l.tag
        assert A.ring_distance(l.quads)[0] == 10.0 and A.reference_range(l.tag[2], l.quads[0]) < 10.0, l.tag
        assert (A.oracle_scan(l) == 10.0).all(), l.tag
    near = _sides(2, 'near', A.OFF_NEAR)
    for (off, sgn), r in near.items():
        for l, c in r:
            f = c['first']
            assert f['near'] == (not (off == 1e-5 and sgn > 0)) and f['kept'] == (sgn < 0), (l.tag, f)
    assert len(_sel(2, 'near', 'diagonal')) >= MIN_BRANCH and all(c['first']['near'] and not c['first']['kept'] for l, c in _sel(2, 'near', 'diagonal'))
    at10, beyond = _sel(2, 'hit', 'at_10'), _sel(2, 'hit', 'beyond')
    assert len(at10) >= MIN_BRANCH and len(beyond) >= MIN_BRANCH
    for l, c in at10 + beyond:                                           # (the ring's other edges are nearer: only the axis beam is looked at)
        ego = l.ego()[0]
        i = int(round(math.atan2(ego[:2, 1].mean(), ego[:2, 0].mean()) / A.PITCH)) % A.NBEAM
        r2, _ = A.exact_ranges(ego, beams=[i])
        assert c['first']['kept'] and i % 30 == 0 and r2[i] is not None and r2[i] >= 100, (l.tag, i)
        assert (r2[i] - 100 < 1e-25) if l.tag[1] == 'at_10' else (r2[i] > 100.25), (l.tag, float(r2[i]))
        assert A.oracle_scan(l)[i] == 10.0                               # the clip
    print('family 2:', dict(tally), {k: len(r) for k, r in near.items()}, 'hit at 10:', len(at10), 'beyond:', len(beyond))


def test_family_3_lots_behind_and_through_the_sensor():
    """Counts (lots): the edge's line meets an axis beam 5e-9, 9e-9, 2e-8, 5e-7 and 2e-6 m behind the sensor in 24 lots each (12 with the
    whole edge behind: the beam it stands behind reads that range at 5e-9 and 9e-9 and not beyond the reference's 1e-8; 12 crossing) -- the edge subtends pi there, so it is wild and paired with all 120 beams; 12 lots with an
    edge through the sensor point (range exactly 0 on 118 beams or more); 32 with the sensor strictly inside a ring (never culled); the
    sensor on an edge's line 16, |sin| = 5e-7 on each side 16 + 16 (not decisive), 2e-6 on each side 16 + 16 (decisive)."""
    for off in A.OFF_BEHIND:
        for form in (0, 1):
            rows = _sel(3, 'behind', off, form)
            assert len(rows) >= MIN_SIDE and all(c['first']['wild'] >= 1 for l, c in rows), (off, form)
            if form == 0:                                                # the whole edge behind: a hit at range `off` on the axis beam it stands
                for l, c in rows:                                        # across iff the reference's 1e-8 lets it count
                    ego = l.ego()[0]
                    i = (int(round(math.atan2(ego[:2, 1].mean(), ego[:2, 0].mean()) / A.PITCH)) + 60) % A.NBEAM
                    assert i % 30 == 0 and (A.oracle_scan(l, [0])[i] < 1e-8) == (off < 1e-8), (l.tag, i, A.oracle_scan(l, [0])[i])
    thr = _sel(3, 'through')
    assert len(thr) >= MIN_BRANCH
    for l, c in thr:
        assert c['first']['wild'] >= 1 and (A.oracle_scan(l) == 0.0).sum() >= 118, l.tag
    ins = _sel(3, 'inside')
    assert len(ins) >= MIN_BRANCH
    for l, c in ins:
        assert c['first']['kept'] and not c['first']['culled'] and (A.oracle_scan(l) < 10).sum() >= 60, l.tag
    on = _sides(3, 'online', (0.0,) + A.OFF_DECISIVE)
    for (s, sgn), rows in on.items():
        for l, c in rows:
            assert c['first']['undecisive'] == (s < 1e-6), (l.tag, c['first'])
    print('family 3:', {k: len(r) for k, r in on.items()}, 'through', len(thr), 'inside', len(ins))


def test_family_4_wild_edges_overflow_the_queue_in_both_halves_of_a_wave_and_in_one():
    """Counts (lots): 20 / 20 / 20 / 40 lots with exactly 1 / 3 / 4 / 8 wild edges (each paired with 120 beams: the branch for more
    than 64 beams of one edge), from three on always one by an end point 0.05 m away and one by subtending > 3.13 rad; 80 lots with
    more pairs than the one-scene queue (384: 4 x 120 already exceed it), 79 waves of the pair kernel with both lots wild (family
    3's wild lots included), 50 with one; 60 of those waves hold more than 512 pairs."""
    small, _ = A.small_and_large()
    cen = {id(l): c for l, c in table()}
    for w in A.WILD_MIX:
        rows = _sel(4, 'wild', w)
        assert len(rows) >= MIN_BRANCH
        for l, c in rows:
            assert c['wild'] == w and c['wide'] == w, (l.tag, c['wild'], c['wide'])
            if w >= 3:
                assert c['wild_vertex'] >= 1 and c['wild_span'] >= 1, l.tag
            if w >= 4:
                assert c['pairs'] > A.LQ_ONE
    over_one = sum(c['pairs'] > A.LQ_ONE for l, c in _sel(4, 'wild'))
    assert over_one >= MIN_BRANCH
    both = one = over = 0
    for i in range(0, len(small) - 1, 2):
        a, b = cen[id(small[i])], cen[id(small[i + 1])]
        both += a['wild'] > 0 and b['wild'] > 0
        one += (a['wild'] > 0) != (b['wild'] > 0)
        over += (a['wild'] > 0 or b['wild'] > 0) and a['pairs'] + b['pairs'] > A.LQ_PAIR
    print('family 4: lots over the one-scene queue', over_one, 'waves with both lots wild', both, 'with one', one, 'of them over the pair queue', over)
    assert both >= MIN_BRANCH and one >= MIN_BRANCH and over >= MIN_BRANCH


CONVEX_SHAPES = ('quad', 'angle_26', 'edge_051')


def test_family_5_shapes_set_and_clear_the_shape_flags():
    """Counts (lots): eleven shapes x both windings x 8 lots of three copies each, all within range and seen from outside: the convex flag
    holds for the quad, the 26-degree corner and the 0.051 m edge (rings culled in all 48 of those lots), not for darts, bow-ties,
    triangles, collinear rings, rings with zero-length edges, the 24-degree corner and the 0.049 m edge; clockwise copies clear the CCW flag."""
    culled = 0
    for name in A.SHAPES:
        for wind in ('ccw', 'cw'):
            rows = _sel(5, 'shape', name, wind)
            assert len(rows) >= MIN_BRANCH, (name, wind)
            for l, c in rows:
                assert c['n_kept'] == 3 and c['wild'] == 0, l.tag
                assert c['nonconvex'] == (0 if name in CONVEX_SHAPES else 3), (l.tag, c['nonconvex'])
                if name in CONVEX_SHAPES:
                    assert c['cw'] == (3 if wind == 'cw' else 0), l.tag
                    culled += c['culled_rings'] > 0
    assert culled >= 6 * MIN_BRANCH
    print('family 5: lots of convex shapes with a culled ring', culled)


def test_family_6_counts_cross_every_chunk_boundary():
    """Counts (lots): 8 lots each with exactly 0, 1, 15, 16, 17, 31, 32 kept rings (small tile) and 33, 63, 64, 65, 128 (large tile),
    with a few more obstacles out of range (half of them inside the near list's box) shuffled among them; 16 lots of 24 / 32 long
    walls with 624 or more ordinary pairs and no wild edge; lots of 255 obstacles with 255 and 131 kept."""
    for kept in A.KEPT_SMALL + A.KEPT_LARGE:
        rows = _sel(6, 'kept', kept)
        assert len(rows) >= MIN_BRANCH
        for l, c in rows:
            assert c['n_kept'] == kept and c['wild'] == 0 and c['n_amb'] == 0, (l.tag, c['n_kept'])
            assert (len(l.quads) <= A.SMALL_TILE) == (kept in A.KEPT_SMALL), l.tag
            assert c['n_near'] > kept or kept in (32, 128), l.tag            # listed as near, then dropped by the ring test
    walls = _sel(6, 'walls')
    assert len(walls) >= MIN_BRANCH and all(c['wild'] == 0 and c['pairs'] > A.LQ_PAIR and len(l.quads) <= A.SMALL_TILE for l, c in walls)
    rng = np.random.default_rng(255)
    for kept in (255, 131):
        assert A.census(A.lot_255(rng, kept))['n_kept'] == kept
    print('family 6: pairs of the wall lots', sorted(c['pairs'] for l, c in walls))


CULL_GATES = ('wild', 'undecisive', 'near_beam', 'thin', 'nonconvex', 'one_facing')


def test_every_gate_of_the_back_face_cull_alone_blocks_it_somewhere():
    """Lots in which a kept ring with both facings is kept from the cull by ONE gate alone (or, last entry, only by showing one
    facing: the sensor inside it).  Measured: wild 111, undecisive 24, near_beam 484, thin 103, nonconvex 116,
    one facing 22; and lots with a culled ring: 1425."""
    lots = collections.Counter()
    for l, c in table():
        for g in CULL_GATES:
            lots[g] += c['cull_blocked_by'].get(g, 0) > 0
        lots['culled'] += c['culled_rings'] > 0
    print('back-face cull, lots per gate that alone blocks it:', dict(lots))
    assert all(lots[g] >= MIN_BRANCH for g in CULL_GATES + ('culled',)), lots


def test_families_1_to_6_are_not_trivially_out_of_range():
    """at least half the lots of families 1-6 have a beam below the range (measured: 1538 of 1572)"""
    rows = [l for l, c in table() if l.fam <= 6]
    below = sum(bool((A.oracle_scan(l) < 10.0).any()) for l in rows)
    print('families 1-6: lots', len(rows), 'with a beam below the range', below)
    assert 2 * below >= len(rows)


# ---- the independent anchor ----------------------------------------------------------------------------------------------------------------
def test_generic_family_oracle_range_is_the_exact_nearest_hit():
    """The oracle's range per beam against the exact nearest hit on the generic family (48 lots x 120 beams).  A (lot, beam) pair
    is CLEAN when no ring vertex lies within 1e-6 rad of the beam and the exact range is not within 1e-6 m of 0 or 10; at least
    90 % of the pairs have to be clean (measured: 5760 of 5760).  Measured largest deviation over the clean pairs: 2.04e-14 m; the bound is 8 x that
    (headroom for a differently rounded libm build)."""
    lots = [l for l, c in table() if l.fam == 7]
    worst, clean, total = 0.0, 0, 0
    for l in lots:
        ego = l.ego()
        r2, root = A.exact_ranges(ego)                                   # every ring: a hit below 10 m lies on a ring the reference keeps
        gap = A.vertex_beam_gap(ego)
        scan = A.oracle_scan(l)
        ok = (gap > 1e-6) & (root > 1e-6) & (root < 10.0 - 1e-6)
        total += A.NBEAM
        clean += int(ok.sum())
        worst = max(worst, float(np.abs(scan[ok] - root[ok]).max(initial=0.0)))
    print(f'generic family: {total} (lot, beam) pairs, clean {clean}, largest deviation of the oracle from the exact range {worst:.3g} m')
    assert clean >= 0.9 * total
    assert worst <= 8 * 2.04e-14


def test_families_1_to_3_decisions_that_exact_arithmetic_fixes():
    """Ring by ring, alone in front of the sensor: a ring whose EXACT distance is >= 10 gives no hit on any beam; a ring whose exact
    distance is < 10 - 1e-9 and that a clean beam crosses (exact range on that beam in (1e-6, 10 - 1e-6), no vertex within 1e-4 rad)
    gives the exact nearest hit on that beam to 1e-9 m.  The second claim is made only where the edge hit first has both coordinate
    extents > 1e-3 m: the reference's coordinate-box test has no tolerance, so on an axis-parallel edge the rounding of the
    quotient decides whether the hit counts (the oracle reproduces that, and loses such hits), and exact arithmetic fixes nothing.
    Measured: 2834 rings, 131 at or beyond the range (14 at exactly 10; one of the 131 is kept all the same, by the rounding of GEOS's distance, and still gives no hit), 2310 with a clean crossing beam (up to three beams per ring: 6779 in all).  Of 531 clean beams
    whose first hit lies on an axis-parallel edge the oracle loses the hit on 87, which is why they are counted and not asserted."""
    far = tie = near = rings = kept_far = beams = axis_beams = axis_lost = 0
    for l, c in table():
        if l.fam > 3:
            continue
        ego = l.ego()
        for r in range(len(ego)):
            rings += 1
            d2 = A.ring_distance2_exact(ego[r])
            if d2 >= 100:
                far += 1
                tie += d2 == 100
                kept_far += bool(c['kept_mask'][r])                       # (GEOS's rounded distance can fall below 10 where the exact one does not)
                assert (A.oracle_scan(l, [r]) == 10.0).all(), (l.tag, r, float(d2))
                continue
            if d2 >= (10 - 1e-9) ** 2:
                continue
            assert c['kept_mask'][r], (l.tag, r)
            fr, edge = A.float_ranges(ego[r])
            gap = A.vertex_beam_gap(ego[r])
            ext = np.abs(np.roll(ego[r], -1, axis=0) - ego[r]).min(axis=1)             # smaller coordinate extent per edge
            clean = (fr > 1e-3) & (fr < 9.99) & (gap > 1e-4)
            scan = None
            for slanted in (True, False):
                cand = np.nonzero(clean & ((ext[edge] > 1e-3) == slanted))[0]
                for i in sorted({int(cand[0]), int(cand[len(cand) // 2]), int(cand[-1])} if len(cand) else ()):   # up to three beams
                    r2, root = A.exact_ranges(ego[r], beams=[i])
                    if r2[i] is None or not 1e-6 < root[i] < 10 - 1e-6:  # not a clean beam after all (an edge through the sensor)
                        continue
                    scan = A.oracle_scan(l, [r]) if scan is None else scan
                    if slanted:
                        assert scan[i] < 10.0 and abs(scan[i] - root[i]) < 1e-9, (l.tag, r, i, scan[i], root[i])
                        beams += 1
                    else:                                                # first hit on an axis-parallel edge: counted, not asserted
                        axis_beams += 1
                        axis_lost += abs(scan[i] - root[i]) >= 1e-9
                near += slanted and len(cand) > 0
    print(f'families 1-3: {rings} rings, at or beyond the range {far} (exactly 10: {tie}; kept all the same by the rounding of the distance: {kept_far}), with a clean crossing beam {near} ({beams} beams looked at); '
          f'clean beams whose first hit is on an axis-parallel edge {axis_beams}, hit lost by the oracle {axis_lost}')
    assert far >= 100 and tie >= MIN_BRANCH and near >= 1000
    assert axis_lost >= MIN_BRANCH                                       # the reason for the restriction: such hits do get lost
