"""The CPU oracle's Reeds-Shepp search on exactly aligned and degenerate poses (tests/rs_degenerate.py) against the reference's
own results (tests/golden/rs_degenerate.npz, written by tests/golden/make_golden_r2.py `rsdegen`).

On these poses words carry segments of length exactly 0 or ~1e-16, the solvers' guards run on their boundaries, and
generate_local_course's trailing pop removes samples that are in use.  The glibc build of the oracle must reproduce the reference
bit for bit in every discrete output; the hope_math build (what the kernels compute) may differ only where the result is the sign
of libm noise.
"""
import numpy as np
import pytest

import rs_degenerate as D
from oracle import oracle as O
from rs_illcond import allowed_results, tie_group_results


@pytest.fixture(scope='module')
def lattice():
    return D.build(max_obst=2)


@pytest.fixture(scope='module')
def fixture(gold, lattice):
    g = gold('rs_degenerate.npz')
    assert int(g['n_cases']) == lattice['n']            # the file belongs to this lattice
    return g


def search(lat, i):
    m = int(lat['n_obst'][i])
    return O.find_rs_path(lat['start'][i], lat['dest'][i], lat['verts'][i, :m], lat['nvert'][i, :m], lat['bbox'][i])


@pytest.fixture(scope='module')
def runs(lattice):
    """every search of the lattice once per oracle form; shared by the tests below and left unchanged"""
    out = {}
    try:
        for name, libm, tail_only in (('libm', True, False), ('hope_math', False, False), ('hope_math_tail_only', False, True)):
            O.use_libm(libm)
            O.rs_pop_mode(tail_only)
            O.rs_used_popped(reset=True)
            res, popped = [], np.zeros(lattice['n'], np.int64)
            for i in range(lattice['n']):
                res.append(search(lattice, i))
                popped[i] = O.rs_used_popped(reset=True)
            out[name] = (res, popped)
    finally:
        O.rs_pop_mode(False)
        O.use_libm(False)
    return out


def zero_segment_among_popped(pose, dest, n_popped):
    """does one of the first `n_popped` words in order of length (tie group of the last one included) hold a segment |l| < 1e-9"""
    a = O.rs_all_paths(pose, dest, D.MAXC)
    order = sorted(range(a['n']), key=lambda k: a['L'][k])
    k = min(n_popped, len(order))
    while k < len(order) and abs(a['L'][order[k]] - a['L'][order[k - 1]]) <= 1e-9 * max(1.0, a['L'][order[k]]):
        k += 1
    idx = order[:k]
    return bool(((np.abs(a['lengths'][idx]) < 1e-9) & (a['ctypes'][idx] >= 0)).any())


def word(r):
    return tuple(int(c) for c in r['ctypes'][:r['nseg']]) if r['found'] else ()


def test_lattice_is_what_the_issue_describes(lattice, fixture):
    lat = lattice
    assert lat['lattice'].max() + 1 == 3 * 8 * 9 * 10 == 2160
    assert 3000 <= lat['n'] <= 8000
    assert set(np.unique(lat['variant'][~lat['gate']])) == {0, 1, 2}
    # gate group: exactly 10.0 and its two float64 neighbours, both t
    g = lat['gate']
    assert sorted(set(lat['gate_d'][g])) == [np.nextafter(10.0, 0.0), 10.0, np.nextafter(10.0, 20.0)]
    assert set(lat['t'][g]) == {1, 2} and (lat['t'][~g] == 2).all()
    # the poses at 4 / maxc = 12.02 m lie beyond the gate (the search itself is still pinned here, the GPU test sees them cleared);
    # the box of the car is clear of the obstacles at both ends (builder's drop rule)
    far = lat['gate_d'][~g] >= 10.0
    assert 0 < far.sum() < 0.2 * far.size and np.abs(lat['gate_d'][~g][far] - 4 / D.MAXC).max() < 1e-12
    for i in np.nonzero(lat['n_obst'] > 0)[0][::37]:
        m = int(lat['n_obst'][i])
        for pose in (lat['start'][i], lat['dest'][i]):
            assert not O.detect_collision(O.create_box(pose), lat['verts'][i, :m], lat['nvert'][i, :m])
    kept = fixture['kept']
    share = kept.mean()
    print(f'rs_degenerate: {lat["n"]} searches, kept by the 1e-6 m margin filter {int(kept.sum())} ({100 * share:.2f} %), '
          f'reference raised IndexError on {int(fixture["ref_error"].sum())}, heap: {fixture["heap"]}')
    assert share >= 0.90
    assert (fixture['margin'][kept] >= 1e-6).all()
    # the degenerate material is there: words with a ~zero segment, searches that go deep, the word of (5, 0, 0) -> (0, 0, 0)
    zero_seg = ((np.abs(fixture['lengths']) < 1e-9) & (fixture['ctypes'] >= 0)).any(axis=1)
    assert zero_seg.sum() > 100 and (fixture['n_tested'] > 1).sum() > 200 and fixture['n_tested'].max() >= 8


def test_glibc_build_has_pythons_hypot(fixture):
    """math.hypot of the interpreter that wrote the fixture, recorded there on 1 500 arguments over seven decades: bit for bit"""
    try:
        O.use_libm(True)
        got = O.math_fn(6, fixture['hypot_x'], fixture['hypot_y'])
    finally:
        O.use_libm(False)
    assert np.array_equal(got, fixture['hypot'])
    # the routine restated in hope_oracle.c is CPython 3.10's; a fixture regenerated under another interpreter has to bring its own
    assert str(fixture['python']).startswith('3.10.'), fixture['python']


def test_glibc_oracle_equals_the_reference_on_every_kept_case(lattice, fixture, runs):
    """found, n_tested, word types and the sample count of every tested word exactly, lengths to 1e-9.  (13 kept cases -- exact-length
    LRSL / RSLR twins, the car diagonal to the goal at 9.5 m -- order by the last bit of `path.L`, which comes from math.hypot:
    CPython's own routine, not glibc's.  The glibc build carries that routine, see test_glibc_build_has_pythons_hypot.)"""
    res, _ = runs['libm']
    g = fixture
    off = g['npts_off']
    for i in np.nonzero(g['kept'])[0]:
        r = res[i]
        assert r['found'] == bool(g['found'][i]), i
        assert r['n_tested'] == int(g['n_tested'][i]), i
        assert np.array_equal(r['npts'], g['npts'][off[i]:off[i + 1]]), i
        assert np.array_equal(r['ctypes'], g['ctypes'][i]), i
        assert np.abs(r['lengths'] - g['lengths'][i]).max() < 1e-9, i
        assert abs(r['L'] - g['L'][i]) < 1e-9, i


def test_hope_math_oracle_differs_only_where_the_result_is_libm_noise(lattice, fixture, runs):
    """hope_math vs the reference: a difference is excused only if both results are reachable under arbitrary tie order / axis
    luck (rs_illcond.allowed_results: twins, axis cases) or the words involved hold a segment with |l| < 1e-9; at most 5 % of the
    kept cases may differ at all.  (Exact tie groups of more than two words -- rs_illcond.tie_group_results -- are twins too.)"""
    res, _ = runs['hope_math']
    g = fixture
    kept = np.nonzero(g['kept'])[0]
    differ, unexcused = [], []
    for i in kept:
        r = res[i]
        gw = tuple(int(c) for c in g['ctypes'][i] if c >= 0) if g['found'][i] else ()
        same = (r['found'] == bool(g['found'][i]) and r['n_tested'] == int(g['n_tested'][i]) and word(r) == gw
                and np.abs(r['lengths'] - g['lengths'][i]).max() < 1e-9)
        if same:
            continue
        differ.append(i)
        m = int(lattice['n_obst'][i])
        allowed = allowed_results(lattice['start'][i], lattice['dest'][i], lattice['verts'][i, :m], lattice['nvert'][i, :m],
                                  lattice['bbox'][i])
        tiny = lambda ln, ct: bool(((np.abs(ln) < 1e-9) & (np.asarray(ct) >= 0)).any())
        if (word(r) in allowed and gw in allowed) or tiny(r['lengths'], r['ctypes']) or tiny(g['lengths'][i], g['ctypes'][i]):
            continue
        twins = tie_group_results(lattice['start'][i], lattice['dest'][i], lattice['verts'][i, :m], lattice['nvert'][i, :m],
                                  lattice['bbox'][i])
        if word(r) in twins and gw in twins:
            continue
        # the words agree and only the pop order before them differs: a ~zero segment in a word that was popped on the way there
        # (the first max(n_tested) words by length, with the exact-length twins of the last of them)
        if zero_segment_among_popped(lattice['start'][i], lattice['dest'][i], max(r['n_tested'], int(g['n_tested'][i]))):
            continue
        unexcused.append(int(i))
    share = len(differ) / len(kept)
    print(f'rs_degenerate: hope_math differs from the reference on {len(differ)} of {len(kept)} kept cases ({100 * share:.2f} %)')
    assert not unexcused, unexcused
    assert share <= 0.05


def test_trailing_pop_is_reached_and_changes_no_result(lattice, fixture, runs):
    """generate_local_course pops trailing samples whose local x is exactly 0.0 (reeds_shepp.py:500-505).  On this lattice that
    removes samples IN USE (the oracle replays it: the glibc test above pins the sample counts; so do the kernels).  On the lattice's
    own obstacles the two forms give the same search result on every case; tests/rs_one_sample.py has the obstacles that tell them
    apart."""
    full, popped = runs['hope_math']
    tail, would_pop = runs['hope_math_tail_only']
    assert np.array_equal(popped, would_pop)
    n_reached = int((popped > 0).sum())
    ref_reached = int((fixture['pop_used'] > 0).sum())
    print(f'rs_degenerate: the trailing pop removes a sample in use on {n_reached} cases (reference run: {ref_reached})')
    assert n_reached > 50 and ref_reached > 50
    changed = [i for i in range(lattice['n'])
               if (full[i]['found'], full[i]['n_tested'], word(full[i])) != (tail[i]['found'], tail[i]['n_tested'], word(tail[i]))
               or not np.array_equal(full[i]['lengths'], tail[i]['lengths'])]
    assert not changed, changed
    # where it fires on a tested word the sample counts do differ: the switch is not a no-op
    assert any(not np.array_equal(full[i]['npts'], tail[i]['npts']) for i in np.nonzero(popped > 0)[0])


def test_reference_overflow_cases_have_a_defined_oracle_result(lattice, fixture, runs):
    """a word that opens with zero-length segments makes the reference write past its own lists while it builds the candidates
    (IndexError): there is no reference result.  The oracle continues as if the lists were long enough; with nothing to compare
    with, what is pinned here is that the two math builds agree on the whole result (found, tested count, word, sample counts,
    lengths), and tests/test_gpu_rs_degenerate.py pins the kernels to the same result."""
    bad = np.nonzero(fixture['ref_error'])[0]
    assert 0 < len(bad) <= 30 and not fixture['kept'][bad].any()
    for i in bad:
        a, b = runs['libm'][0][i], runs['hope_math'][0][i]
        assert a['n_tested'] >= 1 and a['found'] == b['found'] and a['n_tested'] == b['n_tested'], i
        assert np.array_equal(a['ctypes'], b['ctypes']) and np.array_equal(a['npts'], b['npts']), i
        assert np.abs(a['lengths'] - b['lengths']).max() < 1e-9 and abs(a['L'] - b['L']) < 1e-9, i


def test_gate_is_strict_in_distance_and_time(lattice, fixture):
    """car_parking_base.py:293-294: searched iff t > 1 and |pos - dest| < 10, on 10.0 and its two float64 neighbours."""
    ids = np.nonzero(lattice['gate'])[0]
    n = len(ids)
    orc = O.BatchOracle(n, 2)
    orc.set_scenes(np.arange(n), lattice['start'][ids], lattice['dest'][ids], lattice['bbox'][ids], lattice['verts'][ids],
                   lattice['nvert'][ids], lattice['n_obst'][ids])
    orc.t[:] = lattice['t'][ids] - 1                      # the step increments t before the gate reads it
    o = orc.reset_obs(with_rs=True)
    assert (o['status'] == 1).all()
    searched = (lattice['gate_d'][ids] < 10.0) & (lattice['t'][ids] > 1)
    assert searched.sum() == 2 and (~searched).sum() == n - 2
    assert np.array_equal(o['rs_found'] == 1, searched)          # no obstacle: every search finds its first word
    assert fixture['found'][ids].all()
    assert (o['rs_ctypes'][~searched] == -1).all() and (o['rs_lengths'][~searched] == 0).all()
    assert np.array_equal(o['rs_ctypes'][searched], fixture['ctypes'][ids][searched].astype(np.int32))
