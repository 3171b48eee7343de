"""CPU premises of tests/test_gpu_mask_program.py: the lots of tests/mask_program.py reach the branches of the mask stage they are
aimed at -- asserted from the oracle's scan of every lot and the numpy mirror of the stage, for the shipped table and for one on a
0.05 m grid -- and the mirror, until now fed synthetic scan vectors only, gives the oracle's mask (ActionMask.get_steps and
post_process, action_mask.py:166-196) through a lidar scan on every one of them."""
import numpy as np
import pytest

import mask_program as M
from oracle import oracle as O


@pytest.fixture(scope='module', params=list(M.TABLE_SETS))
def prog(request):
    return M.program(request.param)


def test_every_category_reaches_its_floor(prog):
    """the category of a lot is computed from the oracle's scan and the mirror's trace, not taken from the builder"""
    P = prog
    cats, pairs, waves = M.census(P)
    print(f'{P.name}: {len(P.lots)} lots (+ as many twins) generated in {P.seconds:.1f} s, {P.oracle_calls} aiming scans, '
          f'{P.exact_hits} aimed scans equal to a table entry bit for bit')
    print(' lots per category:', dict(sorted(cats.items())))
    print(' straddle pairs per group of bin edges:', dict(sorted(pairs.items())))
    print(' waves of the pair kernel per kind:', dict(sorted(waves.items())))
    assert 2 * len(P.lots) < 4096 and len(P.lots) % 2 == 1              # the small-tile list ends in a wave with one half
    assert all(len(l.quads) <= M.SMALL_TILE for l in P.lots) and all(len(t.quads) > M.SMALL_TILE for t in P.twins)
    assert {l.pose for l in P.lots} == set(M.POSES)
    short = {c: (cats.get(c, 0), f) for c, f in M.FLOORS.items() if cats.get(c, 0) < f}
    assert not short, short
    assert {c: cats.get(c, 0) for c in M.UNREACHABLE} == M.UNREACHABLE          # (the arithmetic reason stands next to each in mask_program)
    short = {g: (pairs.get(g, 0), f) for g, f in M.PAIR_FLOORS.items() if pairs.get(g, 0) < f}
    assert not short, short
    assert sum(pairs.values()) >= M.FLOOR
    short = {k: waves.get(k, 0) for k in M.PAIR_KINDS if waves.get(k, 0) < M.WAVE_FLOOR}
    assert not short, short
    assert P.seconds < 60.0


def test_entry_lots_are_spread_over_beams_actions_and_rows(prog):
    """(a): the lots whose COMPUTED relation to an entry of the deciding beam is the one they were aimed at cover the front, a side,
    the rear and both sides of beam 64, the first, middle and last action of each direction half, and most rows"""
    P = prog
    want = dict(below='a_below', at='a_at', band_in='a_band_in', band_out='a_band_out', above='a_above', exact='a_exact')
    hit = [l.tag for l, f in zip(P.lots, P.info) if l.fam == 'a' and want[l.tag[0]] in f['cats']]
    for rel in M.RELATIONS:
        tags = [t for t in hit if t[0] == rel]
        assert {t[1] for t in tags} >= {0, 30, 60, 63, 64, 90}, rel
        assert {t[2] for t in tags} >= set(M.EDGE_ACTIONS), rel
        assert len({t[3] for t in tags}) >= 5, rel


def test_straddle_pairs_sit_on_both_sides_of_a_bin_edge(prog):
    """for each pair the computed bins differ by one and both scans lie within 1e-12 of the edge; at the last edge one lot has the
    beam active and the other has not"""
    P = prog
    x = [f['x'] for f in P.info]
    found = M.edge_pairs(P.L, x)
    assert len({(i, b) for _n, i, b, _g in found}) >= 60
    for n, i, b, g in found:
        if g == 'last':
            assert P.info[n]['n_act'] == 1 and P.info[n + 1]['n_act'] == 0
    assert {b for _n, _i, b, _g in found} >= {1, 2, 64, 127, 128}
    assert {i for _n, i, _b, _g in found} >= {0, 63, 64, 119}


def test_twins_have_the_scan_and_the_mask_of_their_lots(prog):
    P = prog
    with M.oracle_tables(P.tables):
        for lot, twin, f in zip(P.lots, P.twins, P.info):
            raw = M.scan_of(twin, P.L['hb'])[0]
            assert np.array_equal(raw, f['raw']), lot.tag
            assert np.array_equal(O.get_steps(raw), O.get_steps(f['raw'])), lot.tag


def test_mirror_equals_the_oracle_through_scan_and_post_process(prog):
    """on every lot without a raised tie the mirror's coarse counts through post_process are ActionMask.get_steps of the oracle's own
    lidar; where the tie is raised, the mirror of the exact evaluation is -- and it never differs from the coarse counts
    (mask_program.UNREACHABLE has the reason), so these lots cannot tell whether a kernel raises the tie at all"""
    P = prog
    n_tie = n_visible = 0
    with M.oracle_tables(P.tables):
        for lot, f in zip(P.lots, P.info):
            want = O.get_steps(f['raw'])
            tr = f['trace']
            if tr['tie']:
                n_tie += 1
                exact = M.exact_path_counts(P.L, f['x'])
                n_visible += int((M.post_process(exact) != M.post_process(tr['ms'])).any())
                got = M.post_process(exact)
            else:
                got = M.post_process(tr['ms'])
            assert np.array_equal(got, want), (lot.fam, lot.tag, got, want)
    print(f'{P.name}: {len(P.lots) - n_tie} lots decided by the coarse beams, {n_tie} by the exact evaluation; on {n_visible} of those '
          f'the coarse counts alone would have given another mask')
    assert n_tie >= M.FLOOR and n_visible == M.UNREACHABLE['f_tie_visible']


def test_oracle_tables_are_restored():
    before = {omp: M._held(omp) for omp in (False, True)}
    P = M.program('quantised')
    with M.oracle_tables(P.tables):
        assert all(np.array_equal(M._held(omp)['dist_star'], P.tables['dist_star']) for omp in (False, True))
    assert all(np.array_equal(before[omp][k], M._held(omp)[k]) for omp in before for k in before[omp])
