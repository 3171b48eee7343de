"""-m gpu: the sub-step event search of the step kernels -- where a step stops among its ten sub-step poses -- against the oracle on
the programmed arrivals and collisions of tests/substep_events.py (premise: tests/test_substep_events.py), in every launch form, each
form's routing asserted per scene through ParkingBatch.step_plan (hope_env_step_plan) to be the kernel the form names:

  (a) one launch, kinematics fused in (wave_kinematics)       the last 4 095 scenes of the set
  (b) one launch behind k_kinematics                          the full set (> 4 096 scenes), HOPE_SPLIT_MIN huge
  (c) two launches: k_motion_pair + k_obs_pair on the small-tile chain, k_env_step PART 1 / PART 2 with a 128-obstacle tile on the other
  (d) two launches with STAGE_ONE_SCENE: k_env_step PART 1 / PART 2 with a 32-obstacle tile on the small-tile chain

float64 observations and actions, overlap=True, STAGE_ALL (the two-launch forms need the search), one reset_obs, the uploaded state
(pose, t, accum) on the device and on the oracle, one step; every output and state word equal with tolerance 0."""
import collections
import functools
import os

import numpy as np
import pytest

import substep_events as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

MO = 128
OUTS = ('status', 'done', 'pose', 'reward', 'reward_info', 'lidar', 'action_mask', 'target')
N_FUSED = 4095


def _oracle_step(sc):
    from hope_amd import tables as TB
    from oracle import oracle as O
    n = len(sc['nob'])
    t = TB.all_tables()
    O.set_tables(hull_base=t['hull_base'], beam_a=t['beam_ab'][:, 0], beam_b=t['beam_ab'][:, 1], dist_star=t['dist_star'], omp=True)
    orc = O.BatchOracle(n, MO, omp=True, track_traj=False)
    orc.set_scenes(np.arange(n), sc['start'], sc['dest'], sc['bbox'], sc['verts'], sc['nvert'], sc['nob'])
    orc.reset_obs(with_rs=False)
    orc.pose[:], orc.t[:], orc.accum[:] = sc['pose'], sc['t'], sc['accum']
    o = orc.step(sc['action'], with_rs=False)
    return dict(status=o['status'].copy(), done=(o['status'] != S.CONTINUE).astype(np.uint8), reward=o['reward'].copy(), reward_info=o['reward_info'].copy(),
                lidar=o['lidar'].copy(), action_mask=o['mask'].copy(), target=o['target'].copy(), pose=orc.pose.copy(), t=orc.t.astype(np.int32),
                accum=orc.accum.copy(), substeps=o['substeps'].copy())


@functools.lru_cache(maxsize=None)
def reference():
    """the scene set and the oracle's step from the uploaded state, once; the premise the cases are built on is re-asserted here for
    the scene set (the CPU test asserts it, with its margins, for the table)"""
    sc = S.scene_set()
    ref = _oracle_step(sc)
    assert np.array_equal(ref['substeps'], sc['substeps']) and np.array_equal(ref['status'], sc['status'])
    return sc, ref


def _rows(d, rows):
    return {k: v[rows] for k, v in d.items()}


def _env(sc):
    from hope_amd import ParkingBatch
    n = len(sc['nob'])
    env = ParkingBatch(n, MO, obs_dtype=torch.float64, action_dtype=torch.float64, overlap=True)
    env.set_scene_arrays(np.arange(n), sc['start'], sc['dest'], sc['bbox'], sc['verts'], sc['nob'])
    return env


def _describe(sc, i):
    return f"scene {i}: {sc['kind'][i]} ka {sc['ka'][i]} kc {sc['kc'][i]} n_near {sc['n_near'][i]} (table case {sc['case'][i]})"


def _check(env, sc, ref, tag, rows=None, partner=None):
    torch.cuda.synchronize()
    rows = np.arange(len(sc['nob'])) if rows is None else rows
    state = dict(zip(('pose_state', 't', 'accum'), env.download_state()))
    for k in OUTS + ('pose_state', 't', 'accum'):
        got = (getattr(env, k).cpu().numpy() if k in OUTS else state[k])[rows]
        want = ref['pose' if k == 'pose_state' else k][rows]
        bad = rows[np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]]
        where = [_describe(sc, i) + ('' if partner is None or partner[i] < 0 else '; partner ' + _describe(sc, partner[i])) for i in bad[:6]]
        assert len(bad) == 0, (tag, k, len(bad), where)


def _census(plan):
    return '; '.join(f"tile class {c['tile_class']} (capacity {c['tile_cap']}): {len(c['scenes'])} scenes, motion {c['motion']}, observation {c['obs']}"
                     for c in plan['chains'])


def _routing(plan, n, want, flags):
    """every scene is in exactly one chain, and each chain runs the kernels `want[tile class]` = (tile capacity, motion, observation)"""
    ids = np.concatenate([c['scenes'] for c in plan['chains']])
    assert np.array_equal(np.sort(ids), np.arange(n))
    assert {c['tile_class'] for c in plan['chains']} == set(want) and len(plan['chains']) == len(want)
    for c in plan['chains']:
        assert (c['tile_cap'], c['motion'], c['obs']) == want[c['tile_class']], (c['tile_class'], c['tile_cap'], c['motion'], c['obs'])
    assert {k: plan[k] for k in ('split', 'pipe', 'fuse_kin', 'auto_subs')} == dict(dict(split=False, pipe=False, fuse_kin=False, auto_subs=False), **flags)


def _run(sc, ref, form, split_min, stages_extra, want, flags, after=None):
    from hope_amd import _lib as L
    stages = L.STAGE_ALL | stages_extra
    os.environ['HOPE_SPLIT_MIN'] = split_min
    try:
        env = _env(sc)
        n = env.n
        env.reset_obs(stages=stages)
        env.upload_state(pose=sc['pose'], t=sc['t'], accum=sc['accum'])
        plan = env.step_plan(stages=stages)
        print(f'form {form}: {n} scenes; {_census(plan)}')
        _routing(plan, n, want, flags)
        partner = np.full(n, -1)
        for c in plan['chains']:
            if c['motion'] == 'pair':
                ids, m = c['scenes'], len(c['scenes']) // 2 * 2
                partner[ids[0:m:2]], partner[ids[1:m:2]] = ids[1:m:2], ids[0:m:2]
        # both tile chains see every kind; the kind census per chain goes with the kernel census
        for c in plan['chains']:
            kinds = collections.Counter(sc['kind'][c['scenes']])
            print(f"  tile class {c['tile_class']}: {dict(sorted(kinds.items()))}")
            assert set(kinds) == set(S.KINDS)
        a = torch.from_numpy(sc['action']).to(env.device)
        env.step(a, stages=stages)
        _check(env, sc, ref, form, partner=partner)
        if after:
            after(env, plan, a, stages, partner)
        env.close()
    finally:
        os.environ.pop('HOPE_SPLIT_MIN', None)


def test_form_a_one_launch_with_the_kinematics_fused_in():
    full, ref_full = reference()
    rows = np.arange(len(full['nob']) - N_FUSED, len(full['nob']))
    sc, ref = S.subset(full, rows), _rows(ref_full, rows)
    assert set(sc['case']) == set(full['case']) and (sc['n_near'] > 32).any()          # every table case, the 40-obstacle lots included
    k = 'one_launch_fused_kin'
    _run(sc, ref, 'a', '1000000000', 0, {0: (32, k, 'in_step'), 1: (MO, k, 'in_step')}, dict(fuse_kin=True))


def test_form_b_one_launch_behind_k_kinematics():
    sc, ref = reference()
    assert len(sc['nob']) > 4096
    _run(sc, ref, 'b', '1000000000', 0, {0: (32, 'one_launch', 'in_step'), 1: (MO, 'one_launch', 'in_step')}, {})


def _pair_coverage(sc, plan):
    """form (c), from the plan's lists: all 64 ordered pairs of half classes; every kind next to a partner with no event, an earlier
    event and a later event (K7 stops at sub-step 0: "earlier" is a partner that stops there too); the last wave's second half empty"""
    (c0,) = [c for c in plan['chains'] if c['motion'] == 'pair']
    ids = c0['scenes']
    assert len(ids) % 2 == 1
    a, b = ids[0:len(ids) - 1:2], ids[1:len(ids):2]
    assert (sc['half_class'][ids] >= 0).all()
    classes = collections.Counter(zip(sc['half_class'][a].tolist(), sc['half_class'][b].tolist()))
    assert len(classes) == len(S.HALF_CLASSES) ** 2, sorted(set((x, y) for x in range(8) for y in range(8)) - set(classes))
    seen = set()
    for x, y in ((a, b), (b, a)):
        ex, ey = sc['event'][x], sc['event'][y]
        rel = np.where(ey == S.NUM_STEP, 'none', np.where(ey < ex, 'earlier', np.where(ey > ex, 'later', 'same')))
        seen |= set(zip(sc['kind'][x].tolist(), rel.tolist()))
    need = {(k, r) for k in S.KINDS[1:] for r in ('none', 'earlier', 'later')} - {('K7', 'earlier')} | {('K7', 'same')}
    assert not need - seen, sorted(need - seen)
    print(f'  pair waves {len(a)} + 1 half-empty; ordered half-class pairs {len(classes)} (rarest {min(classes.values())} waves); '
          f'(kind, partner event) combinations {len(seen)}')


def test_form_c_two_launches_pair_kernels_and_large_tile():
    sc, ref = reference()
    n = len(sc['nob'])

    def after(env, plan, a, stages, partner):
        _pair_coverage(sc, plan)
        # once more from the same uploaded state, one half of two pair waves in three silenced (and some large-tile scenes)
        before = {k: getattr(env, k).cpu().numpy().copy() for k in OUTS}
        env.upload_state(pose=sc['pose'], t=sc['t'], accum=sc['accum'])
        active = np.ones(n, np.uint8)
        for c in plan['chains']:
            ids = c['scenes']
            active[ids[0::6]] = 0                                 # first halves of waves 0, 3, ...
            active[ids[3::6]] = 0                                 # second halves of waves 1, 4, ...
        env.step(a, active=torch.from_numpy(active).to(env.device), stages=stages)
        on, off = np.nonzero(active)[0], np.nonzero(active == 0)[0]
        _check(env, sc, ref, 'c, half of many pairs silenced', rows=on, partner=partner)
        torch.cuda.synchronize()
        for k in OUTS:
            assert np.array_equal(getattr(env, k).cpu().numpy()[off], before[k][off]), ('silenced', k)
        pose, t, acc = env.download_state()
        assert np.array_equal(pose[off], sc['pose'][off]) and np.array_equal(t[off], sc['t'][off]) and np.array_equal(acc[off], sc['accum'][off])
        print(f'  silenced {len(off)} scenes of {n}: outputs and state words kept; the other {len(on)} equal the oracle')

    _run(sc, ref, 'c', '1', 0, {0: (32, 'pair', 'pair'), 1: (MO, 'split_one_scene', 'split_one_scene')}, dict(split=True), after)


def test_form_d_two_launches_one_scene_kernels_on_the_small_tile():
    from hope_amd import _lib as L
    sc, ref = reference()
    k = 'split_one_scene'
    _run(sc, ref, 'd', '1', L.STAGE_ONE_SCENE, {0: (32, k, k), 1: (MO, k, k)}, dict(split=True))


def _bound_row(O, pose, dest):
    """a record of hope_debug_geom fn 9: x, y, cos, sin of the pose, centre of the dest box, cos, sin of its heading"""
    B = O.create_box(dest)
    cs = lambda h: (float(O.math_fn(1, [h])[0]), float(O.math_fn(0, [h])[0]))
    return [pose[0], pose[1], *cs(pose[2]), 0.5 * (B[0, 0] + B[2, 0]), 0.5 * (B[0, 1] + B[2, 1]), *cs(dest[2])]


def test_k4_poses_pass_the_devices_arrival_bound():
    """K4 is about poses whose overlap is computed (the slab bound of arrival_possible passes) although the ratio stays under 0.95, and
    that a collision then cuts off: counted with the device's own bound (hope_debug_geom fn 9) -- some for every kc, and among them
    the pose the step retreats from (without it no stale overlap could be left behind).  K7 likewise: the start pose passes the bound
    in the variant with the dest box over it, and in no case of the variant with the dest box far away"""
    import ctypes as C
    from hope_amd import _lib as L
    from oracle import oracle as O
    rows, key = [], []
    for c in S.table():
        if c['kind'] == 'K4':
            Q = S.extended_poses(c['pose'], c['action'], S.NUM_STEP)
            for k in range(c['kc'] + 1):                          # the poses the walk examines: 0 .. kc
                rows.append(_bound_row(O, Q[k + 1], c['dest']))
                key.append((c['kc'], k))
        elif c['kind'] == 'K7':
            rows.append(_bound_row(O, c['pose'], c['dest']))
            key.append((c['tag'], -1))
    a = torch.from_numpy(np.ascontiguousarray(rows, np.float64)).cuda()
    out = torch.full((len(rows),), -77, dtype=torch.int32, device='cuda')
    L.check(L.load_library().hope_debug_geom(9, len(rows), 0, C.c_void_p(a.data_ptr()), C.c_void_p(out.data_ptr()), None), 'hope_debug_geom')
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert set(np.unique(got)) <= {0, 1}
    passing, cut, total = collections.Counter(), collections.Counter(), collections.Counter()
    for (kc, k), g in zip(key, got):
        passing[kc] += int(g)
        total[kc] += 1
        cut[kc] += int(g) if k == kc else 0
    print('K4 poses that pass the arrival bound, per kc (all examined poses / the pose retreated from):',
          {kc: (passing[kc], cut[kc]) for kc in range(S.NUM_STEP)})
    print('K7 start poses that pass the arrival bound:', {k: (passing[k], total[k]) for k in passing if isinstance(k, str)})
    for kc in range(S.NUM_STEP):
        assert passing[kc] > 0 and cut[kc] > 0, kc
    assert passing['K7 dest over the start pose'] == total['K7 dest over the start pose'] > 0
    assert passing['K7 dest far'] == 0 and total['K7 dest far'] > 0
