"""The premise of tests/test_gpu_motion_reward.py, on the CPU: the oracle, stepped once from the uploaded state of every case of
tests/motion_reward_cases.py, ends with the programmed status after ten sub-steps, and takes the branch the case is meant to hit --
which side of the fold of angle_diff, which accum branch, which dnorm branch, inside or outside the 5.2 m reach of k_post, arrival or
not -- decided in exact rational arithmetic (fractions) on the case's own doubles, with the margin each leaves.  The values of the
tiny-term cells come from a search that emulates the three operations of the device's division by 20 exactly.  Every cell is filled;
the scene set puts 0 / 1 / 16 / 17 / 33 / 64 clipping lanes into the first six k_post waves of both tile chains."""
import collections
import functools
from fractions import Fraction

import numpy as np
import pytest

import motion_reward_cases as M
import substep_events as S
from oracle import oracle as O

# pi to 60 digits: the fold of angle_diff is decided against this rational, |error| < 1e-59
PI_Q = Fraction('3.14159265358979323846264338327950288419716939937510582097494')
FOLD_DECIDED = 1e-12        # the branch is asserted where the exact angle is at least this far from pi / 2 (acos(cos .) errs by < 3e-16 there)


@functools.lru_cache(maxsize=None)
def stepped():
    tab = M.table()
    return tab, M.oracle_step(M.case_arrays(tab))


def exact_fold(delta):
    """|delta| reduced to [0, pi] exactly (what acos(cos(delta)) approximates) -> (angle, angle - pi / 2) as Fractions"""
    a = abs(Fraction(float(delta))) % (2 * PI_Q)
    a = a if a <= PI_Q else 2 * PI_Q - a
    return a, a - PI_Q / 2


def oracle_fold(delta):
    d = float(O.math_fn(5, [float(O.math_fn(1, [delta])[0])])[0])
    return d, d < M.PI / 2


def test_the_search_finds_where_the_three_operations_differ_from_the_division():
    """q0 = RN(x / 20 rounded reciprocal), r = RN(x - 20 q0), RN(q0 + r R) in exact arithmetic against x / 20.0: equal on ordinary
    terms, different at every X = 30 + 40 k subnormal ulps (x / 20 is a tie there: the division rounds to even, the chain down) and
    at a fraction of a percent of the x in [1, 64) 2^-1022 -- the table's tiny terms"""
    found, n_low, n_ord = M.div20_search()
    print(f'division by 20: {n_low} of 20000 random x in [1, 64) 2^-1022 differ, {n_ord} of 20000 in +-0.2; kept {[x.hex() for x in found[:4]]}')
    assert n_ord == 0 and n_low > 0 and len(found) >= 3
    for k in range(8):
        x = (30 + 40 * k) * M.SUB
        assert M.div20_emulated(x) != x / 20.0 and M.div20_emulated(-x) != -x / 20.0, k
    assert M.div20_emulated(31 * M.SUB) == 31 * M.SUB / 20.0
    assert M.div20_emulated(2.0 ** -900) == 2.0 ** -900 / 20.0
    tiny = [c for c in M.table() if c['cell'] in ('tiny', 'tiny sin')]
    differ = [c for c in tiny if M.div20_emulated(c['term']) != c['term'] / 20.0]
    print(f'tiny-term cases: {len(tiny)}, of them where the three operations differ from the division: {len(differ)}')
    assert len(differ) >= 20 and {c['cell'] for c in differ} == {'tiny', 'tiny sin'}
    assert any(c['term'] < 0 for c in differ) and any(c['term'] > 0 for c in differ)


def test_tiny_terms_add_up_as_the_plain_division_says():
    """the oracle's final position of a tiny-term case is the start plus 200 times the quotient term / 20.0, added one by one (exact
    while the sum stays subnormal), the term being the double the table programmed"""
    tab, ref = stepped()
    n = 0
    for i, c in enumerate(tab):
        if c['cell'] not in ('tiny', 'tiny sin') or abs(c['term']) > 2.0 ** -1000:
            continue
        axis = 0 if c['cell'] == 'tiny' else 1
        want = float(c['pose'][axis])
        for _ in range(200):
            want += c['term'] / 20.0
        assert float(ref['pose'][i][axis]) == want, (c['tag'], ref['pose'][i])
        if abs(c['term']) < 2.0 ** -1060:
            assert Fraction(want) == 200 * Fraction(c['term'] / 20.0)
        n += 1
    assert n >= 30


def test_status_substeps_and_time_are_the_programmed_ones():
    tab, ref = stepped()
    for i, c in enumerate(tab):
        assert ref['status'][i] == c['expect'], (c['tag'], ref['status'][i])
        assert ref['substeps'][i] == M.NUM_STEP, c['tag']                # ten sub-steps kept (the arrival is found at the tenth pose)
        assert ref['t'][i] == c['t'] + 1
        assert np.isfinite(ref['pose'][i]).all() and np.isfinite(ref['target'][i]).all() and np.isfinite(ref['reward_info'][i]).all()
    census = collections.Counter((c['cell'], int(ref['status'][i])) for i, c in enumerate(tab))
    print('status census (cell, status):', dict(sorted(census.items())))
    assert census[('time', M.OUTTIME)] >= 1 and census[('time', M.CONTINUE)] >= 4 and census[('overlap', M.ARRIVED)] >= 2
    assert {c['t'] + 1 for c in tab if c['cell'] == 'time'} == {1, 2, 199, 200, 201}


def test_arrival_or_not_with_its_margin():
    """the ratio of every pose of every case whose dest is near, as check_arrived computes it: above 0.95 at the final pose of the
    programmed arrival only, and never within 1e-3 of the threshold"""
    tab, ref = stepped()
    worst = 1.0
    for i, c in enumerate(tab):
        if c['cell'] not in ('overlap', 'accum', 'target'):
            continue
        r = S.ratios(M.poses_of(c['pose'], c['action']), c['dest'])
        worst = min(worst, float(np.abs(r - 0.95).min()))
        assert (r[:-1] <= 0.95).all() and (r[-1] > 0.95) == (c['expect'] == M.ARRIVED), (c['tag'], r)
    print(f'arrival: smallest |ratio - 0.95| over all examined poses {worst:.3e}')
    assert worst > 1e-3


def test_the_fold_side_with_its_margin():
    """angle_diff(heading, dest heading) = acos(cos(d)) folded at pi / 2, d the double the subtraction returns: the exact angle
    (fractions, pi to 60 digits) decides the side where it is clear of the fold; on the fold (d = pi / 2 as a double and its
    neighbours: 6e-17, 1.6e-16 and 2.8e-16 from pi / 2) the side is the oracle's own, printed -- and the programmed differences
    are exact, so the device subtracts to the same double"""
    tab, ref = stepped()
    rows, sides = [], collections.Counter()
    for i, c in enumerate(tab):
        if c['cell'] != 'fold':
            continue
        for which, h in (('previous', c['pose'][2]), ('current', ref['pose'][i][2])):
            d = h - c['dest'][2]
            ang, margin = exact_fold(d)
            got, below = oracle_fold(d)
            if abs(margin) >= FOLD_DECIDED:
                assert below == (margin < 0), (c['tag'], which, float(margin))
            assert abs(Fraction(got) - ang) < Fraction(3e-8)      # (bounded tightly against 50 digits below)
            rows.append((abs(float(margin)), c['tag'], which, below))
            if which == c['fold_which'] or c['fold_which'] == 'both':
                sides[(c['fold_which'], 'below' if below else 'at or above')] += 1
                if c['fold_delta'] == 0 or 1 < abs(c['fold_delta']) < 4:    # the deltas on the fold and at its ends
                    assert c['fold_exact'] and d == c['fold_delta'], (c['tag'], which, d, c['fold_delta'])
    print('fold sides (pose programmed, side the oracle takes):', dict(sorted(sides.items())))
    print('closest to the fold:', [(f'{m:.2e}', t, w, 'below' if b else 'at or above') for m, t, w, b in sorted(rows)[:8]])
    for which in ('current', 'previous', 'both'):
        assert sides[(which, 'below')] >= 4 and sides[(which, 'at or above')] >= 4
    assert sum(1 for m, *_ in rows if m < 1e-15) >= 12


def test_the_accum_branch_with_its_margin():
    """box_union_reward < accum ? 0 : (accum = it, it - previous accum): the uploaded accum against the `bur` of the first pass, as
    Fractions; equal and 1 ulp below take the second branch (difference 0 and 1 ulp), 1 ulp above and 1.5 the first"""
    tab, ref = stepped()
    kinds = collections.Counter()
    for i, c in enumerate(tab):
        if c['cell'] != 'accum':
            continue
        bur, acc = Fraction(c['first_bur']), Fraction(c['accum'])
        margin = bur - acc
        if margin < 0:
            assert ref['reward_info'][i][4] == 0.0 and ref['accum'][i] == c['accum'], c['tag']
        else:
            assert ref['accum'][i] == c['first_bur'] and Fraction(float(ref['reward_info'][i][4])) == margin, c['tag']
        assert (margin == 0) == (c['accum_kind'] == 'equal') and (margin < 0) == (c['accum_kind'] in ('1 ulp above bur', 'far above'))
        kinds[(c['accum_kind'], 'zeroed' if margin < 0 else 'taken')] += 1
    print('accum branches (uploaded accum against the first pass, branch):', dict(sorted(kinds.items())))
    assert len(kinds) == 4 and min(kinds.values()) >= 6
    first = [c for c in tab if c['cell'] in ('overlap', 'target') and c['bur'] > 0]
    assert len(first) >= 10                                       # accum 0: the first pass itself


def test_the_dnorm_branch_with_its_margin():
    tab, ref = stepped()
    seen = collections.Counter()
    for c in tab:
        if c['cell'] != 'dnorm':
            continue
        d2 = sum((Fraction(float(c['dest'][k])) - Fraction(float(c['start'][k]))) ** 2 for k in (0, 1))
        side = 'below' if d2 < 100 else 'above' if d2 > 100 else 'exactly 10'
        seen[(c['dnorm'], side)] += 1
        want = {'below': 'below', 'above': 'above', 'exactly 10': 'exactly 10', '10 - 1 ulp': 'below', '10 + 1 ulp': 'above'}[c['dnorm']]
        assert side == want, (c['tag'], float(d2 - 100))
        if 'ulp' in c['dnorm']:
            assert abs(float(d2 - 100)) < 1e-13
    print('dnorm branches:', dict(sorted(seen.items())))
    assert len(seen) == 5


def test_inside_or_outside_the_reach_of_k_post_with_its_margin():
    """centre distance of the final hull's box and the dest box against 5.2, squared, as Fractions of the boxes' doubles (the device
    forms the same centres from the same vertices: its rounding is ~1e-15, the programmed margins are 1e-9)"""
    tab, ref = stepped()
    seen = collections.Counter()
    for i, c in enumerate(tab):
        if c['cell'] != 'overlap' or 'reach' not in c:
            continue
        d2 = M.centre_dist2_exact(ref['pose'][i], c['dest'])
        margin = float(d2) ** 0.5 - M.REACH
        inside = d2 <= Fraction(M.REACH) ** 2
        assert inside == (c['reach'] < M.REACH + 5e-10) and abs(margin - (c['reach'] - M.REACH)) < 1e-12, (c['tag'], margin)
        assert c['clip'] == inside and not M.slab_margin(ref['pose'][i], c['dest'])[0]
        seen[(c['reach'], bool(inside))] += 1
    print('reach (programmed centre distance, inside):', dict(sorted(seen.items())))
    assert len(seen) == 4 and min(seen.values()) >= 2
    # which overlap cases k_post clips itself (the slab bound fails within reach) and which the walk computed (it passes)
    by = collections.Counter((c.get('overlap'), c['clip']) for c in tab if c['cell'] == 'overlap')
    print('overlap cases (kind, clipped by k_post):', dict(sorted(by.items(), key=str)))
    for r in (0.05, 0.5, 0.93):
        assert by[(f'ratio {r}', True)] >= 2
    assert by[('ratio 0.945', False)] >= 2 and by[('none, within reach', True)] >= 2


def test_oracle_against_50_digit_arithmetic():
    """tanh(t / 2000) and angle_diff of every case against mpmath at 50 digits.  Bounds: tanh -- 2 ulp of the result (hope_math's
    claim for its elementary functions is < 1 ulp; the argument's division adds half); angle_diff -- the cosine carries an absolute
    error of up to 2^-52 (its rounding and the function's), which acos magnifies by 1 / sin(angle): 2^-51 / sin(angle) + 4 ulp of
    pi, and never more than sqrt(2 2^-51) = 3e-8 (acos(1 - e) = sqrt(2 e))"""
    mp = pytest.importorskip('mpmath')
    mp.mp.dps = 50
    tab, ref = stepped()
    worst_t, worst_a = 0.0, (0.0, 0.0)
    for i, c in enumerate(tab):
        if ref['status'][i] != M.CONTINUE:
            continue
        t = ref['t'][i]
        exact = -mp.tanh(mp.mpf(int(t)) / 2000)
        err = abs(mp.mpf(float(ref['reward_info'][i][0])) - exact)
        worst_t = max(worst_t, float(err / abs(exact)))
        assert err <= 2 * 2.0 ** -52 * abs(exact), (c['tag'], float(err))
        for h in (c['pose'][2], ref['pose'][i][2]):
            d = h - c['dest'][2]
            got, _ = oracle_fold(d)
            exact = mp.acos(mp.cos(mp.mpf(float(d))))
            err = float(abs(mp.mpf(got) - exact))
            bound = min(2.0 ** -51 / max(float(mp.sin(exact)), 1e-300), (2 * 2.0 ** -51) ** 0.5) + 4 * 2.0 ** -52 * M.PI
            assert err <= bound, (c['tag'], d, err, bound)
            if err / bound > worst_a[1]:
                worst_a = (err, err / bound)
    print(f'against 50 digits: tanh worst relative error {worst_t:.3e}; acos(cos(.)) worst error {worst_a[0]:.3e} ({worst_a[1]:.3f} of its bound)')


def test_every_cell_is_filled_and_the_scene_set_programs_the_clip_census():
    tab = M.table()
    cells = collections.Counter(c['cell'] for c in tab)
    print(f'cell census: {len(tab)} cases; per cell {dict(sorted(cells.items()))}')
    assert set(cells) == {'controls', 'chain', 'zero', 'tiny', 'tiny sin', 'time', 'dnorm', 'fold', 'overlap', 'accum', 'target'}
    big = collections.Counter(c['cell'] for c in tab if len(c['quads']) > 32)
    print(f'  in 40-obstacle lots: {dict(sorted(big.items()))}')
    assert set(big) == set(cells) and all(len(c['quads']) <= 3 or len(c['quads']) == M.N_LARGE for c in tab)
    # controls: every value of the list as steer, as speed and as both
    vals = {repr(float(v)) for v in M.control_values()}
    for role in ('steer', 'speed', 'both'):
        assert {c['tag'].split()[-1] for c in tab if c['tag'].startswith(f'controls {role}')} >= vals, role
    assert len(vals) == 16
    for cases, name in ((M.f32_cases(), 'float32'), (M.phys_cases(), 'physical')):
        per = collections.Counter(c['cell'] for c in cases)
        print(f'  {name} subset: {len(cases)} cases {dict(sorted(per.items()))}')
        assert not any(np.isnan(c['action']).any() for c in cases)
    assert all((c['action'].astype(np.float32).astype(np.float64) == c['action']).all() for c in M.f32_cases())
    assert any(np.signbit(c['action'][1]) and c['action'][1] == 0 for c in M.phys_cases())
    assert not any(np.isnan(c[k]).any() for c in tab for k in ('action', 'pose', 'dest', 'start'))
    heads = {c['pose'][2] for c in tab if c['cell'] == 'chain'}
    assert heads == set(M.START_HEADINGS) and len(heads) == 17
    assert {c['target'] for c in tab if c['cell'] == 'target'} >= {'atan2(0, 0)', 'behind, rdy +0.0', 'behind, rdy -0.0', 'ahead', 'left', 'right',
                                                                  'float32 tie 8 + 2^-21', 'float32 tie 8 + 3 2^-21'}
    # the scene set: both chains' lists begin with the census block, in the full set and in the 4 095 scenes of the fused form
    sc, m, rows = M.scene_set()
    n = len(sc['nob'])
    assert n == M.N_SCENES > 4096 and m % 16 != 0 and (n - m) % 16 != 0 and (sc['nob'][:n - 2 * sum(big.values())] <= 32).all()
    for name, clip, mm in (('full set', sc['clip'], m), ('fused form', sc['clip'][rows], len(rows) - int(M.CLS1_FRAC * len(rows)))):
        for lo in (0, mm):
            got = [int(clip[lo + 64 * w:lo + 64 * (w + 1)].sum()) for w in range(len(M.CENSUS))]
            assert tuple(got) == M.CENSUS, (name, lo, got)
            for w, k in enumerate(M.CENSUS):
                if k in (17, 33):                                 # mixed: no run of clipping lanes longer than 2
                    lanes = clip[lo + 64 * w:lo + 64 * (w + 1)].astype(int)
                    assert max(len(r) for r in ''.join(map(str, lanes)).split('0')) <= 2
        assert sc['clip_clear'][:64 * len(M.CENSUS)].all() and sc['clip_clear'][m:m + 64 * len(M.CENSUS)].all()
        print(f'  {name}: small-tile list {mm} scenes, large-tile list {len(clip) - mm}; clipping lanes of the first six k_post waves of each {M.CENSUS}')
    for lo, hi in ((0, m), (m, n)):                               # every cell in both chains
        assert {tab[k]['cell'] for k in sc['case'][lo:hi]} == set(cells)
    assert set(sc['case'][rows]) == set(range(len(tab)))
