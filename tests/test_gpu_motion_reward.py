"""-m gpu: kinematics (action rescale and clip, heading chain, ordered position sums), reward and target representation of the step
kernels against the oracle on the programmed actions and poses of tests/motion_reward_cases.py (premise:
tests/test_motion_reward_cases.py), in every launch form, each form's routing asserted per scene through ParkingBatch.step_plan:

  (a) one launch, kinematics fused in (wave_kinematics)       4 095 scenes of the set
  (b) one launch behind k_kinematics                          the full set (4 101 scenes), HOPE_SPLIT_MIN huge
  (c) two launches: k_motion_pair + k_obs_pair on the small-tile chain, k_env_step PART 1 / PART 2 with a 128-obstacle tile on the other
  (d) two launches with STAGE_ONE_SCENE: k_env_step PART 1 / PART 2 with a 32-obstacle tile on the small-tile chain

One reset_obs, the uploaded state (pose, t, accum) on the device and on the oracle, one step; every output and every state word equal
as BIT PATTERNS (-0.0 is not +0.0), tolerance 0.  In every form the plan's list order puts 0 / 1 / 16 / 17 / 33 / 64 clipping lanes into
the first six k_post waves of both chains (asserted with the premise's clip flags).  Besides: float32 observations in form (b); the
float32 action paths and ACTION_PHYSICAL on their subsets; scenes silenced through active= in k_kinematics' block patterns."""
import collections
import functools
import os

import numpy as np
import pytest

import motion_reward_cases as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

MO = 128
OUTS = ('status', 'done', 'pose', 'reward', 'reward_info', 'lidar', 'action_mask', 'target')
STATE = ('pose_state', 't', 'accum')


def _tables():
    from hope_amd import tables as TB
    from oracle import oracle as O
    t = TB.all_tables()
    O.set_tables(hull_base=t['hull_base'], beam_a=t['beam_ab'][:, 0], beam_b=t['beam_ab'][:, 1], dist_star=t['dist_star'])


@functools.lru_cache(maxsize=None)
def reference():
    """the scene set and the oracle's step from the uploaded state, once"""
    _tables()
    sc, m, rows = M.scene_set()
    ref = M.oracle_step(sc)
    assert np.array_equal(ref['status'], sc['expect']) and (ref['substeps'] == M.NUM_STEP).all()
    return sc, ref, m, rows


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def _rows(d, rows):
    return {k: v[rows] for k, v in d.items()}


def _env(sc, obs=None, act=None, **kw):
    from hope_amd import ParkingBatch
    n = len(sc['nob'])
    env = ParkingBatch(n, MO, obs_dtype=obs or torch.float64, action_dtype=act or torch.float64, overlap=True, **kw)
    env.set_scene_arrays(np.arange(n), sc['start'], sc['dest'], sc['bbox'], sc['verts'], sc['nob'])
    return env


def _check(env, sc, ref, tag, rows=None, tab=None):
    """every output and state word of the scenes `rows` against the oracle's, as bit patterns; float32 outputs against the oracle's
    doubles rounded once"""
    torch.cuda.synchronize()
    tab = tab or M.table()
    rows = np.arange(len(sc['nob'])) if rows is None else rows
    state = dict(zip(STATE, env.download_state()))
    differing, problems = 0, []
    for k in OUTS + STATE:
        got = (getattr(env, k).cpu().numpy() if k in OUTS else state[k])[rows]
        want = ref['pose' if k == 'pose_state' else k][rows]
        if got.dtype == np.float32:
            want = want.astype(np.float32)
        assert got.dtype == want.dtype, (k, got.dtype, want.dtype)
        diff = (_bits(got) != _bits(want)).reshape(len(got), -1)
        bad = rows[np.nonzero(diff.any(axis=1))[0]]
        differing += int(diff.sum())
        where = [f"scene {i}: {tab[sc['case'][i]]['tag']} got {np.ravel(got[list(rows).index(i)])[:5]} want {np.ravel(want[list(rows).index(i)])[:5]}" for i in bad[:5]]
        if len(bad):
            problems.append((k, len(bad), where))
    print(f'  {tag}: {len(rows)} scenes, {differing} differing words')
    assert not problems, (tag, problems)


def _census(plan):
    return '; '.join(f"tile class {c['tile_class']} (capacity {c['tile_cap']}): {len(c['scenes'])} scenes, motion {c['motion']}, observation {c['obs']}"
                     for c in plan['chains'])


def _routing(plan, n, want, flags):
    ids = np.concatenate([c['scenes'] for c in plan['chains']])
    assert np.array_equal(np.sort(ids), np.arange(n))
    assert {c['tile_class'] for c in plan['chains']} == set(want) and len(plan['chains']) == len(want)
    for c in plan['chains']:
        assert (c['tile_cap'], c['motion'], c['obs']) == want[c['tile_class']], (c['tile_class'], c['tile_cap'], c['motion'], c['obs'])
    assert {k: plan[k] for k in ('split', 'pipe', 'fuse_kin', 'auto_subs')} == dict(dict(split=False, pipe=False, fuse_kin=False, auto_subs=False), **flags)


def _silence(env, sc, ref, plan, a, stages, tag):
    """once more from the same uploaded state with scenes silenced in the patterns of k_kinematics' 16-scene blocks (list order of
    each chain): a whole block, the first scene of a block, the last scene of a block, one lane group (one scene) inside a block --
    the kept scenes equal the oracle, the silenced ones keep every output and state word"""
    n = env.n
    torch.cuda.synchronize()
    before = {k: getattr(env, k).cpu().numpy().copy() for k in OUTS}
    env.upload_state(pose=sc['pose'], t=sc['t'], accum=sc['accum'])
    active = np.ones(n, np.uint8)
    for c in plan['chains']:
        ids = c['scenes']
        assert len(ids) > 16 * 40
        active[ids[48:64]] = 0                                    # a whole block (the block returns early)
        active[ids[96]] = 0                                       # the first scene of a block
        active[ids[16 * 9 + 15]] = 0                              # the last scene of a block
        active[ids[16 * 12 + 5]] = 0                              # one lane group inside a block
        active[ids[16 * 30 + 1:16 * 30 + 16:2]] = 0               # every other lane group of a block
        active[ids[len(ids) // 16 * 16:]] = 0                     # the partial block at the end of the list
    env.step(a, active=torch.from_numpy(active).to(env.device), stages=stages)
    on, off = np.nonzero(active)[0], np.nonzero(active == 0)[0]
    _check(env, sc, ref, tag + ', kept scenes', rows=on)
    for k in OUTS:
        assert np.array_equal(_bits(getattr(env, k).cpu().numpy()[off]), _bits(before[k][off])), ('silenced', k)
    pose, t, acc = env.download_state()
    assert np.array_equal(_bits(pose[off]), _bits(sc['pose'][off])) and np.array_equal(t[off], sc['t'][off]) and np.array_equal(_bits(acc[off]), _bits(sc['accum'][off]))
    print(f'  silenced {len(off)} scenes of {n}: outputs and state words kept; the other {len(on)} equal the oracle')


def _run(sc, ref, form, split_min, stages_extra, want, flags, obs=None, silence=False):
    from hope_amd import _lib as L
    stages = L.STAGE_ALL | stages_extra
    tab = M.table()
    os.environ['HOPE_SPLIT_MIN'] = split_min
    try:
        env = _env(sc, obs=obs)
        n = env.n
        env.reset_obs(stages=stages)
        env.upload_state(pose=sc['pose'], t=sc['t'], accum=sc['accum'])
        plan = env.step_plan(stages=stages)
        print(f'form {form}: {n} scenes; {_census(plan)}')
        _routing(plan, n, want, flags)
        cells = {c['cell'] for c in tab}
        for c in plan['chains']:
            per = collections.Counter(sc['cell'][c['scenes']])
            print(f"  tile class {c['tile_class']}: {dict(sorted(per.items()))}")
            assert set(per) == cells                              # both chains see every cell
            assert len(c['scenes']) % 16 != 0                     # a partial k_kinematics block at the end of each list
        waves = M.post_wave_census(plan, sc['clip'])
        for c, w in zip(plan['chains'], waves):
            print(f"  tile class {c['tile_class']}: clipping lanes per k_post wave, first six {w[:6]}, all waves {dict(sorted(collections.Counter(w).items()))}")
            assert tuple(w[:len(M.CENSUS)]) == M.CENSUS and sc['clip_clear'][c['scenes'][:64 * len(M.CENSUS)]].all()
        a = torch.from_numpy(sc['action']).to(env.device)
        env.step(a, stages=stages)
        _check(env, sc, ref, f'form {form}')
        if silence:
            _silence(env, sc, ref, plan, a, stages, f'form {form}')
        env.close()
    finally:
        os.environ.pop('HOPE_SPLIT_MIN', None)


def test_form_a_one_launch_with_the_kinematics_fused_in():
    full, ref_full, _m, rows = reference()
    sc, ref = M.subset(full, rows), _rows(ref_full, rows)
    assert len(rows) == 4095 and set(sc['case']) == set(full['case']) and (sc['nob'] > 32).any()
    k = 'one_launch_fused_kin'
    _run(sc, ref, 'a', '1000000000', 0, {0: (32, k, 'in_step'), 1: (MO, k, 'in_step')}, dict(fuse_kin=True), silence=True)


def test_form_b_one_launch_behind_k_kinematics():
    sc, ref, _m, _rows_a = reference()
    assert len(sc['nob']) > 4096
    _run(sc, ref, 'b', '1000000000', 0, {0: (32, 'one_launch', 'in_step'), 1: (MO, 'one_launch', 'in_step')}, {}, silence=True)


def test_form_b_with_float32_observations():
    """the oracle's doubles rounded once (the distances on a float32 tie among them); the pose output and the state stay float64"""
    sc, ref, _m, _rows_a = reference()
    tie = [i for i, k in enumerate(sc['case']) if 'float32 tie' in M.table()[k]['tag']]
    d = ref['target'][tie, 0]
    assert len(tie) >= 6 and (np.abs(d.astype(np.float32).astype(np.float64) - d) == 2.0 ** -21).all()      # half a float32 ulp at 8: a tie
    _run(sc, ref, 'b, float32 observations', '1000000000', 0, {0: (32, 'one_launch', 'in_step'), 1: (MO, 'one_launch', 'in_step')}, {}, obs=torch.float32)


def test_form_c_two_launches_pair_kernels_and_large_tile():
    sc, ref, _m, _rows_a = reference()
    _run(sc, ref, 'c', '1', 0, {0: (32, 'pair', 'pair'), 1: (MO, 'split_one_scene', 'split_one_scene')}, dict(split=True), silence=True)


def test_form_d_two_launches_one_scene_kernels_on_the_small_tile():
    from hope_amd import _lib as L
    sc, ref, _m, _rows_a = reference()
    k = 'split_one_scene'
    _run(sc, ref, 'd', '1', L.STAGE_ONE_SCENE, {0: (32, k, k), 1: (MO, k, k)}, dict(split=True))


def _subset_step(cases, ref, act_dtype, stages_extra=0, split_min=None, **kw):
    from hope_amd import _lib as L
    sc = M.case_arrays(cases)
    stages = L.STAGE_ALL | stages_extra
    if split_min:
        os.environ['HOPE_SPLIT_MIN'] = split_min
    try:
        env = _env(sc, act=act_dtype, **kw)
        env.reset_obs(stages=stages)
        env.upload_state(pose=sc['pose'], t=sc['t'], accum=sc['accum'])
        print(f'{env.n} scenes; {_census(env.step_plan(stages=stages))}')
        a = torch.from_numpy(sc['action'].astype(np.float32 if act_dtype == torch.float32 else np.float64)).to(env.device)
        env.step(a, stages=stages)
        _check(env, sc, ref, 'subset', tab=cases)
        env.close()
    finally:
        if split_min:
            os.environ.pop('HOPE_SPLIT_MIN', None)


@pytest.mark.parametrize('split_min', ['1000000000', '1'], ids=['fused kinematics', 'behind k_kinematics'])
def test_float32_actions_with_float64_rescale(split_min):
    """a float32 action buffer without ACTION_RESCALE_F32: the float32 values rescaled in float64, as the oracle's wrapper step does"""
    _tables()
    cases = M.f32_cases()
    _subset_step(cases, M.oracle_step(M.case_arrays(cases)), torch.float32, split_min=split_min)


@pytest.mark.parametrize('split_min', ['1000000000', '1'], ids=['fused kinematics', 'behind k_kinematics'])
def test_float32_actions_with_float32_rescale(split_min):
    """ACTION_RESCALE_F32: the reference's float32 Box arithmetic (env_wrapper.py:46-47, numpy's float32 here), then CarParking.step
    itself (the oracle's physical step) on the float32 result; the last-bit values make the two rescales differ"""
    _tables()
    cases = M.f32_cases()
    sc = M.case_arrays(cases)
    low, high = np.array([-M.STEER_HI, -M.SPEED_HI], np.float32), np.array([M.STEER_HI, M.SPEED_HI], np.float32)
    phys = np.clip(sc['action'].astype(np.float32), np.float32(-1), np.float32(1)) * (high - low) / np.float32(2) + (high + low) / np.float32(2)
    assert phys.dtype == np.float32
    ref = M.oracle_step(sc, physical=True, action=phys.astype(np.float64))
    other = M.oracle_step(sc)
    assert (ref['pose'] != other['pose']).any(axis=1).sum() >= 6      # the two arithmetics do differ on this subset
    _subset_step(cases, ref, torch.float32, split_min=split_min, rescale_f32=True)


@pytest.mark.parametrize('split_min', ['1000000000', '1'], ids=['fused kinematics', 'behind k_kinematics'])
def test_physical_actions(split_min):
    """ACTION_PHYSICAL float64 against the oracle's physical step: beyond the valid range, the range ends +-1 ulp, a speed of -0.0"""
    from hope_amd import _lib as L
    _tables()
    cases = M.phys_cases()
    _subset_step(cases, M.oracle_step(M.case_arrays(cases), physical=True), torch.float64, stages_extra=L.ACTION_PHYSICAL, split_min=split_min)
