"""The premise of tests/test_gpu_substep_events.py, on the CPU: the oracle, stepped once from the uploaded state of every case of
tests/substep_events.py, stops at the sub-step, on the pose and with the status the table says; the margins the cases are built with
hold (so no case rests on the arrival threshold's last bits, on the collision test's robust path or on the rounding of the near
list's boxes); the near list has exactly the programmed length; every cell of the table is filled."""
import collections
import functools

import numpy as np

import substep_events as S
import touching_scenes as T
from oracle import oracle as O

MO = 128


@functools.lru_cache(maxsize=None)
def stepped_table():
    tab = S.table()
    n = len(tab)
    orc = O.BatchOracle(n, MO, omp=True, track_traj=False)
    verts, nob = np.zeros((n, MO, 4, 2)), np.array([len(c['quads']) for c in tab], np.int32)
    for i, c in enumerate(tab):
        if c['quads']:
            verts[i, :nob[i]] = c['quads']
    orc.set_scenes(np.arange(n), np.array([c['start'] for c in tab]), np.array([c['dest'] for c in tab]), np.array([c['bbox'] for c in tab]),
                   verts, np.full((n, MO), 4, np.int32), nob)
    orc.pose[:] = [c['pose'] for c in tab]
    orc.t[:] = [c['t'] for c in tab]
    orc.accum[:] = [c['accum'] for c in tab]
    o = orc.step(np.array([c['action'] for c in tab]), with_rs=False)
    return tab, orc, {k: v.copy() for k, v in o.items()}


def test_the_oracle_stops_where_the_table_says():
    tab, orc, o = stepped_table()
    for i, c in enumerate(tab):
        Q = S.extended_poses(c['pose'], c['action'], S.NUM_STEP)
        assert o['substeps'][i] == c['substeps'], (i, S.cell(c), o['substeps'][i], c['substeps'])
        assert np.array_equal(orc.pose[i], Q[c['final'] + 1]), (i, S.cell(c))
        assert o['status'][i] == c['status'], (i, S.cell(c), c['tag'], o['status'][i], c['status'])
        assert orc.t[i] == c['t'] + 1
    census = collections.Counter((c['kind'], int(o['status'][i])) for i, c in enumerate(tab))
    print('status census (kind, status):', dict(sorted(census.items())))
    for kind, status in (('K5', S.OUTBOUND), ('K5', S.CONTINUE), ('K5', S.ARRIVED), ('K6', S.OUTTIME), ('K6', S.CONTINUE), ('K6', S.ARRIVED),
                         ('K6', S.OUTBOUND), ('K4', S.CONTINUE), ('K7', S.CONTINUE)):
        assert census[(kind, status)] > 0, (kind, status)


def test_the_margins_hold():
    """arrival: start ratio <= 0.947, the first pose above 0.95 is ka, nothing within 0.003 of 0.95; collision: a vertex >= 1 mm inside
    the hull of pose kc and one outside, the quad >= 2 mm off the start hull and the hulls before kc, every other obstacle >= 1 cm off
    every hull or >= 1 mm beyond the box around them; near miss: best ratio of the ten poses in (0.90, 0.945); bounds: the edge is the final pose's coordinate or its
    neighbouring float64 on the inner side"""
    tab, orc, o = stepped_table()
    nv = np.full(1, 4, np.int32)
    for i, c in enumerate(tab):
        Q = S.extended_poses(c['pose'], c['action'], S.NUM_STEP)
        r = S.ratios(Q, c['dest'])
        if c['ka'] >= 0:
            assert r[0] <= S.START_RATIO_MAX and (np.abs(r[1:] - S.ARRIVE_RATIO) >= S.RATIO_BAND).all(), (i, r)
            assert np.nonzero(r[1:] > S.ARRIVE_RATIO)[0][0] == c['ka'], (i, r)
        else:
            assert r.max() < 0.945, (i, S.cell(c), r)
        if c['kind'] == 'K4' or c['tag'] == 'K7 dest over the start pose':
            assert 0.90 < r[1:].max() < 0.945, (i, r)
            assert S.slab_bound(Q[c['kc'] + 1 if c['kind'] == 'K4' else 0], c['dest'])     # the pose cut off / stayed on: its overlap is computed
        if c['tag'] == 'K7 dest far':
            assert not S.slab_bound(Q[0], c['dest'])
        quads = np.array(c['quads']).reshape(-1, 4, 2)
        hit = np.zeros(len(quads), bool)
        if c['kc'] >= 0:
            depth = np.array([S.inside_depth(Q[c['kc'] + 1], q) for q in quads])
            hit = depth.max(axis=1) >= S.HIT_DEPTH
            assert hit.sum() == 1 and depth[hit].min() <= -S.HIT_DEPTH, (i, S.cell(c))
            hq = quads[hit][0]
            assert O.detect_collision(O.create_box(Q[c['kc'] + 1]), hq[None], nv)
            d = T.hull_distance(Q[:c['kc'] + 1], hq.mean(axis=0)[None]).min() - np.linalg.norm(hq - hq.mean(axis=0), axis=1).max()
            assert d >= S.HIT_CLEAR, (i, S.cell(c), d)               # (the quad lies in that disc about its centre)
            assert not any(O.detect_collision(O.create_box(p), hq[None], nv) for p in Q[:c['kc'] + 1])
        if (~hit).any():
            rest = quads[~hit]
            cen, rad = rest.mean(axis=1), np.sqrt(((rest - rest.mean(axis=1, keepdims=True)) ** 2).sum(-1)).max(axis=1)
            beyond = S.near_flags(T.hulls_box(Q), rest)[1]        # >= 1 mm beyond the box around the hulls: as far off every hull
            assert (beyond | (T.hull_distance(Q, cen).min(axis=0) - rad >= 0.0099)).all(), (i, S.cell(c))
        if c['edge'] >= 0:
            F = Q[c['final'] + 1][c['edge'] // 2]
            assert c['bbox'][c['edge']] == (np.nextafter(F, np.inf if c['edge'] % 2 == 0 else -np.inf) if c['edge_ulp'] else F)


def test_the_near_list_has_the_programmed_length():
    tab = S.table()
    for i, c in enumerate(tab):
        Q = S.extended_poses(c['pose'], c['action'], S.NUM_STEP)
        box = T.hulls_box(Q)
        assert len(c['quads']) <= max(32, c['n_near'])
        if not c['quads']:
            assert c['n_near'] == 0
            continue
        near, far = S.near_flags(box, c['quads'])
        assert (near ^ far).all() and near.sum() == c['n_near'] == T.near_count(Q, c['quads']), (i, S.cell(c))


def test_every_cell_is_filled_and_the_scene_set_pairs_every_class():
    tab = S.table()
    cells = collections.Counter(S.cell(c) for c in tab)
    need = S.required_cells()
    assert not need - set(cells) and min(cells[k] for k in need) >= 2
    by_kind = collections.Counter(c['kind'] for c in tab)
    print(f'cell census: {len(tab)} cases in {len(cells)} cells ({len(need)} required, each >= 2 replicas); per kind {dict(sorted(by_kind.items()))}')
    for kind in ('K1', 'K2', 'K3'):
        per_n = collections.Counter(c['n_near'] for c in tab if c['kind'] == kind)
        print(f'  {kind}: cases per near-list length {dict(sorted(per_n.items()))}')
    print('  K4 (kc, accum):', sorted(collections.Counter((c['kc'], c['accum']) for c in tab if c['kind'] == 'K4').items()))
    print('  K5 / K6 / K7 variants:', dict(sorted(collections.Counter(c['tag'] for c in tab if c['kind'] in ('K5', 'K6', 'K7')).items())))
    assert {(c['kc'], c['accum']) for c in tab if c['kind'] == 'K4'} == {(k, a) for k in range(10) for a in (0.0, 0.3, 0.9)}
    assert {(c['final_name'], c['edge'], c['edge_ulp']) for c in tab if c['kind'] == 'K5' and c['final_name'] != 'walk'} == \
        {(f, e, u) for f in ('pose 9', 'retreat', 'start') for e in range(4) for u in (False, True)}
    assert {(c['kind'], c['scale']) for c in tab} >= {(k, s) for k in S.KINDS for s in T.SCALES}
    speeds = np.array([c['action'][1] for c in tab])
    assert (np.abs(speeds) >= 0.4).all() and (speeds > 0).sum() > 300 and (speeds < 0).sum() > 300
    # the scene set: odd, above 4 096, the small-tile chain (the ids below the handed-over share) odd too and free of 40-obstacle lots
    sc = S.scene_set()
    n = len(sc['case'])
    m = n - int(0.42 * n)
    assert n > 4096 and n % 2 == 1 and m % 2 == 1 and (sc['n_near'][:m] <= 32).all() and (sc['nob'][:m] <= 32).all()
    assert set(np.unique(sc['case'])) == set(range(len(tab)))
    pairs = {(int(a), int(b)) for a, b in zip(sc['half_class'][0:m - 1:2], sc['half_class'][1:m:2])}
    assert len(pairs) == 64, len(pairs)
    for rows in (slice(0, m), slice(m, n)):                       # every cell in both tile chains
        assert not need - {S.cell(tab[k]) for k in sc['case'][rows]}
    print(f'scene set: {n} scenes, small-tile chain {m}, large-tile chain {n - m}, of them with 40 obstacles {int((sc["n_near"] > 32).sum())}')
