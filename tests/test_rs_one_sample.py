"""The premises of tests/rs_one_sample.py as exact counts, and the CPU oracle on its cases against the reference's own results
(tests/golden/rs_one_sample.npz, written by tests/golden/make_golden_r2.py `rsonesample`).

The counts are properties of the generator (no RNG) and of the oracle's hope_math build; a change of either that moves one of them
has to be looked at, not waved through.  tests/test_gpu_rs_one_sample.py runs the same cases through the kernels.
"""
import collections

import numpy as np
import pytest

import rs_one_sample as R
from oracle import oracle as O
from rs_illcond import allowed_results, tie_group_results
from test_rs_degenerate import zero_segment_among_popped

# schedule categories a kept case of family (a) can fall into (rs_one_sample.labels), with the number of kept cases that do
CATEGORIES = {
    'stride1': 1856, 'stride2': 564, 'coarse': 2206, 'rest': 214, 'coarse_lane0': 447, 'coarse_lane63': 143, 'rest_lane0': 37,
    'carried': 271, 'later_window': 790, 'sample0': 300, 'final': 185,
    'seg0_first': 125, 'seg0_last': 173, 'seg1_first': 277, 'seg1_last': 222, 'seg2_first': 312, 'seg2_last': 380,
    'seg3_first': 137, 'seg3_last': 175, 'seg4_first': 3, 'seg4_last': 7,
}
# ... and what the schedule cannot produce, with the reason (rs_one_sample.windows derives the bounds)
UNREACHABLE = {
    'stride3': 'a tested window holds at most 63 carried + 63 new + the final sample = 127 samples: stride = ceil(n / 64) <= 2',
    'rest_lane63': 'a rest round holds n - ceil(n / 2) <= 63 samples: lanes 0 .. 62',
    'bad1_equal': 'no lattice word has a first segment whose length equals a sample of the pd chain bit for bit',
    'table_end': 'no lattice word has a first segment of 256 samples: the first-segment table is never exhausted',
}


@pytest.fixture(scope='module')
def cases():
    return R.cases()


@pytest.fixture(scope='module')
def fixture(gold, cases):
    g = gold('rs_one_sample.npz')
    assert int(g['n_cases']) == sum(c['family'] in ('a', 'b') for c in cases[0])      # the file belongs to this generator
    assert str(g['heap']).startswith('heapdict 1.0.1')
    return g


def word(r):
    return tuple(int(c) for c in r['ctypes'][:r['nseg']]) if r['found'] else ()


def run(cs, libm):
    out = []
    try:
        O.use_libm(libm)
        for c in cs:
            out.append(R.search(c['pose'], c['goal'], c['rings'], c['bbox']))
    finally:
        O.use_libm(False)
    return out


@pytest.fixture(scope='module')
def runs(cases):
    """every search of families (a) and (b) once per math build; shared and left unchanged"""
    ab = [c for c in cases[0] if c['family'] in ('a', 'b')]
    return ab, {'libm': run(ab, True), 'hope_math': run(ab, False)}


def test_family_sizes_and_shares(cases):
    cs, st = cases
    fam = collections.Counter(c['family'] for c in cs)
    print('rs_one_sample:', dict(fam), st)
    a = st['a']
    # 11 816 placements; exactly one colliding sample on 4 677, two adjacent ones on 821; the search's result changes on all of
    # those 5 498; 647 of them depend on the libm (rs_one_sample.libm_independent) and are dropped; every second one is kept
    assert (a['placements'], a['one'], a['two'], a['changed'], a['libm_noise']) == (11816, 4677, 821, 5498, 647)
    assert st['a_all'] == 4851 and a['not_restated'] == 2          # (2 poses where l * maxc does not round-trip: skipped)
    assert dict(fam) == {'a': 2426, 'b': 475, 'c': 2640}
    n_hit = collections.Counter(c['n_hit'] for c in cs if c['family'] == 'a')
    assert dict(n_hit) == {1: 2070, 2: 356}
    assert collections.Counter(c['depth'] for c in cs if c['family'] == 'a') == {0: 1625, 1: 476, 2: 325}


def test_every_schedule_category_is_hit_or_recorded_unreachable(cases):
    """the place in the walk's schedule where the kernel has to see the collision of a kept case (the restated walk, which must also
    find the word the oracle finds)"""
    cs, _ = cases
    cat = collections.Counter()
    bad1 = collections.Counter()
    max_first, max_samples, max_found = 0, 0, 0
    for c in cs:
        if c['family'] != 'a':
            continue
        r = c['result']
        wf = c['walk_found']
        assert (c['words'][wf]['types'] if wf >= 0 else ()) == word(r)
        if r['found']:
            max_found = max(max_found, len(c['words'][wf]['pds']))
        ev = c['events'][c['depth']]
        assert ev is not None                                                  # the target word is condemned ...
        if ev['kind'] == 'bad1':                                               # ... by the first-segment cache, unsampled, or
            bad1['target_skipped'] += 1
        else:                                                                  # ... at the diamond's sample(s) and nowhere else
            assert len(ev['samples']) <= c['n_hit']
            cat.update(R.labels(c['words'][c['depth']], ev))
        for e in c['events']:
            if e is not None and e['kind'] == 'bad1':
                bad1['skips'] += 1
                bad1['equal'] += e['equal']
        for w in c['words']:
            max_first = max(max_first, int((w['segs'] == 0).sum()))
            max_samples = max(max_samples, len(w['pds']))
    print('rs_one_sample categories:', dict(cat), dict(bad1), 'longest first segment', max_first, 'longest word', max_samples,
          'longest found word', max_found)
    assert dict(cat) == CATEGORIES
    assert all(v > 0 for v in CATEGORIES.values())
    assert not set(UNREACHABLE) & set(cat) and 'stride3' not in cat and 'rest_lane63' not in cat
    # a first-segment sample that condemns a later word through bad1: the later word is skipped unsampled
    assert bad1['target_skipped'] == 6 and bad1['skips'] == 160 and bad1['equal'] == 0
    assert (max_first, max_samples, max_found) == (98, 187, 185)               # (the 256-entry table and queue are never the limit)
    assert max_first < R.TAB and max_samples < R.TAB


def test_trailing_pop_changes_results(cases):
    cs, st = cases
    b = st['b']
    print('rs_one_sample trailing pop:', b)
    # 88 free poses have a tested word that loses a sample in use; 660 diamonds on their goal hulls, 185 of them libm noise; on 63 of
    # the other 475 the reference's form and the tail-only form of the oracle return different results
    assert (b['poses'], b['placements'], b['libm_noise'], b['differ']) == (88, 660, 185, 63)
    assert b['differ'] > 0
    assert b['pop_hist'] == {0: 6437, 1: 111, 2: 8}                             # words of all free poses by the number of popped samples
    assert b['max_popped'] == 2                                                 # the largest number of samples in use popped from one word
    assert sum(c['differs'] for c in cs if c['family'] == 'b') == b['differ']


def test_glibc_oracle_equals_the_reference(fixture, runs):
    """found, n_tested, word types and the sample count of every tested word exactly, lengths to 1e-9"""
    ab, res = runs
    g = fixture
    off = g['npts_off']
    assert int((g['pop_used'] > 0).sum()) > 400
    for i, r in enumerate(res['libm']):
        assert r['found'] == bool(g['found'][i]), i
        assert r['n_tested'] == int(g['n_tested'][i]), i
        assert np.array_equal(r['npts'], g['npts'][off[i]:off[i + 1]]), i
        assert np.array_equal(r['ctypes'], g['ctypes'][i]), i
        assert np.abs(r['lengths'] - g['lengths'][i]).max() < 1e-9, i
        assert abs(r['L'] - g['L'][i]) < 1e-9, i


def test_hope_math_oracle_differs_only_where_the_result_is_libm_noise(fixture, runs):
    """the tie rules of tests/test_rs_degenerate.py: a difference is excused only if both results are reachable under arbitrary tie
    order / axis luck, the words hold a segment with |l| < 1e-9, or a word popped on the way does"""
    ab, res = runs
    g = fixture
    differ, unexcused = [], []
    for i, (c, r) in enumerate(zip(ab, res['hope_math'])):
        gw = tuple(int(t) for t in g['ctypes'][i] if t >= 0) if g['found'][i] else ()
        if (r['found'] == bool(g['found'][i]) and r['n_tested'] == int(g['n_tested'][i]) and word(r) == gw
                and np.abs(r['lengths'] - g['lengths'][i]).max() < 1e-9):
            continue
        differ.append(i)
        v = np.asarray(c['rings'], dtype=np.float64).reshape(-1, 4, 2)
        nv = np.full(len(v), 4, np.int32)
        allowed = allowed_results(c['pose'], c['goal'], v, nv, c['bbox'])
        tiny = lambda ln, ct: bool(((np.abs(ln) < 1e-9) & (np.asarray(ct) >= 0)).any())
        if (word(r) in allowed and gw in allowed) or tiny(r['lengths'], r['ctypes']) or tiny(g['lengths'][i], g['ctypes'][i]):
            continue
        twins = tie_group_results(c['pose'], c['goal'], v, nv, c['bbox'])
        if word(r) in twins and gw in twins:
            continue
        if zero_segment_among_popped(c['pose'], c['goal'], max(r['n_tested'], int(g['n_tested'][i]))):
            continue
        unexcused.append(i)
    share = len(differ) / len(ab)
    print(f'rs_one_sample: hope_math differs from the reference on {len(differ)} of {len(ab)} cases ({100 * share:.2f} %)')
    assert not unexcused, unexcused
    assert share <= 0.05


def test_margin_verdicts_flip_with_the_sign_of_the_gap(cases):
    """family (c): the oracle's verdict on the pose a square was built on is a collision iff the gap is negative, for every
    |gap| >= 1e-6 -- except where the hull is exactly axis-parallel (straight behind a goal heading 0 or pi / 2): there the reference's
    tolerance-free box test needs the intersection's coordinate to equal the edge's bit for bit, and nothing ever collides."""
    cs, _ = cases
    kinds = collections.Counter()
    flat = 0
    for c in cs:
        if c['family'] != 'c':
            continue
        kinds[c['kind']] += 1
        if c['kind'] in ('wall', 'corner_wall') or abs(c['gap']) < 1e-6:
            continue
        if c['kind'] == 'box':
            hit = not R.search(c['pose'], c['goal'], c['rings'], c['bbox'])['found']
        else:
            hit = bool(R.oracle_hits(np.asarray(c['at'])[None], c['rings'], c['bbox'])[0])
        if c['start'] == 'behind' and c['straight'] and c['goal'][2] in (0.0, np.pi / 2):
            flat += 1
            assert not hit
        else:
            assert hit == (c['gap'] < 0), (c['kind'], c['start'], c['straight'], c['gap'], c['sine'], c['goal'][2])
    assert dict(kinds) == {'square': 1080, 'corner': 360, 'front_arc': 480, 'wall': 480, 'corner_wall': 120, 'box': 120}
    assert flat == 160
