"""-m gpu: the lidar scan, and the action mask and status next to it, on the lots of tests/lidar_adversarial.py -- beam-aligned,
range-tie, sensor-adjacent, wild, oddly shaped and chunk-boundary lots -- against the oracle with tolerance 0.

The oracle runs the reference's plain loop of 120 beams over all edges; the device puts a stack of filters in front of it
(hope_amd/csrc/hope_step_kernel.h "---- lidar", hope_amd/csrc/hope_obs_pair.h) that drawn lots decide on the easy side.  The
premise -- which lot reaches which branch -- is asserted on the CPU by tests/test_lidar_adversarial.py; here every launch form of
tests/test_gpu_exact_geometry.FORMS has to give the oracle's bits on reset_obs, on a zero-action step (the observation launch's
stage_near path at an unchanged pose) and on a moving step; the pair kernels have to equal the one-scene kernels, the cull must
change no bit, a turnover onto these lots has to give the new episode's first scan, float32 observations have to be the rounded
float64 ones exactly, and a handle of 255 obstacles has to agree as well.  A mismatch is reported as (family, tag, scene,
beam, got, want)."""
import functools
import os

import numpy as np
import pytest

import lidar_adversarial as A

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

MO = 128
CONTINUE = 1
FORMS = {'one_launch': ('1000000000', False), 'two_launch_pair_kernels': ('1', False), 'two_launch_large_tile': ('1', True)}
OBS = ('lidar', 'action_mask', 'status')


def _stages():
    from hope_amd import _lib as L
    return L.STAGE_MOTION | L.STAGE_OBS | L.STAGE_REWARD


def _oracle(sc, mo=MO):
    from hope_amd import tables as TB
    from oracle import oracle as O
    n = len(sc['nob'])
    t = TB.all_tables()
    O.set_tables(hull_base=t['hull_base'], beam_a=t['beam_ab'][:, 0], beam_b=t['beam_ab'][:, 1], dist_star=t['dist_star'], omp=True)
    orc = O.BatchOracle(n, mo, omp=True, track_traj=False)
    orc.set_scenes(np.arange(n), sc['start'], sc['dest'], sc['bbox'], sc['verts'], sc['nvert'], sc['nob'])
    return orc


def _snap(orc, o):
    return dict(lidar=o['lidar'].copy(), action_mask=o['mask'].copy(), status=o['status'].copy(), pose=orc.pose.copy())


@functools.lru_cache(maxsize=None)
def reference():
    """the lots (small-tile class first, an odd number, then the large-tile class), and the oracle's reset observation, zero-action
    step and moving step on them, once"""
    small, large = A.small_and_large()
    lots = small + large
    assert len(small) % 2 == 1 and len(lots) <= 2048
    sc = A.arrays(lots, MO)
    sc['n_small'] = len(small)
    orc = _oracle(sc)
    ref = [_snap(orc, orc.reset_obs(with_rs=False))]
    from oracle import oracle as O
    ties = [l for l in lots if l.tag[:2] == ('tie', 'computed_10')]      # with the device's tables in the oracle: dropped, a hit below 10 if kept
    assert len(ties) >= 8 and all(O.lidar_fast(l.quads, [4])[l.tag[2]] < 10.0 and A.ring_distance(l.quads)[0] == 10.0 for l in ties)
    rng = np.random.default_rng(77)
    zero = np.zeros((len(lots), 2))
    move = np.where((ref[0]['status'] == CONTINUE)[:, None], rng.uniform(-0.5, 0.5, (len(lots), 2)), 0.0)   # lots whose start pose is free
    ref.append(_snap(orc, orc.step(zero, with_rs=False)))
    ref.append(_snap(orc, orc.step(move, with_rs=False)))
    assert (ref[0]['status'] == CONTINUE).sum() >= 0.5 * len(lots)
    assert (np.abs(ref[2]['pose'] - ref[1]['pose']).max(axis=1) > 0).sum() >= 0.4 * len(lots)      # the moving step moves
    return lots, sc, (zero, move), ref


def _env(sc, mo=MO, large=False, dtype=None, rows=None):
    from hope_amd import ParkingBatch
    rows = np.arange(len(sc['nob'])) if rows is None else rows
    n = len(rows)
    env = ParkingBatch(n, mo, obs_dtype=dtype or torch.float64, action_dtype=torch.float64, overlap=True)
    env.set_scene_arrays(np.arange(n), sc['start'][rows], sc['dest'][rows], sc['bbox'][rows], sc['verts'][rows], sc['nob'][rows])
    if large:
        env.set_draw_class(np.arange(n), 1)
    return env


def _mismatches(lots, got, want, k):
    bad = np.argwhere((got != want).reshape(len(got), -1))
    return [(lots[i].fam, lots[i].tag, int(i), int(j), got.reshape(len(got), -1)[i, j], want.reshape(len(got), -1)[i, j]) for i, j in bad[:6]], \
        sorted({lots[i].fam for i, _ in bad}), k


def _check(env, lots, ref, tag, cast=None):
    torch.cuda.synchronize()
    for k in OBS:
        got = getattr(env, k).cpu().numpy()
        want = ref[k] if cast is None or k == 'status' else ref[k].astype(cast)
        n_bad = int((got != want).sum())
        assert n_bad == 0, (tag, k, n_bad) + _mismatches(lots, got, want, k)
    if cast is None:
        assert np.array_equal(env.download_state()[0], ref['pose']), tag


def _run(env, lots, acts, ref, tag, cast=None):
    env.reset_obs(stages=_stages())
    _check(env, lots, ref[0], (tag, 'reset_obs'), cast)
    for a, r, name in zip(acts, ref[1:], ('zero-action step', 'moving step')):
        env.step(torch.from_numpy(a).to(env.device), stages=_stages())
        _check(env, lots, r, (tag, name), cast)


@pytest.mark.parametrize('form', list(FORMS))
def test_adversarial_lots_equal_the_oracle_in_every_launch_form(form):
    """lidar, action_mask and status with tolerance 0 on reset_obs, a zero-action step and one moving step (small random actions
    where the start pose is free)"""
    lots, sc, acts, ref = reference()
    split, large = FORMS[form]
    os.environ['HOPE_SPLIT_MIN'] = split
    try:
        env = _env(sc, large=large)
        _run(env, lots, acts, ref, form)
        below = (ref[0]['lidar'] + env.tables['hull_base'][None] < 10.0).any(axis=1)
        print(f'{form}: lots {len(lots)} (small-tile class {sc["n_small"]}), with a beam below the range {int(below.sum())}, '
              f'start pose free {int((ref[0]["status"] == CONTINUE).sum())}: 0 mismatches on 3 observations')
        env.close()
    finally:
        os.environ.pop('HOPE_SPLIT_MIN', None)


def test_pair_kernels_equal_the_one_scene_kernels_on_adversarial_lots():
    """the small-tile class: two lots per wave (wild lots in both halves of a wave, and in one) against STAGE_ONE_SCENE, every output
    and the state bit for bit"""
    from hope_amd import _lib as L
    lots, sc, acts, ref = reference()
    rows = np.arange(sc['n_small'])
    os.environ['HOPE_SPLIT_MIN'] = '1'
    try:
        envs = [_env(sc, rows=rows) for _ in range(2)]
        for e, extra in zip(envs, (0, L.STAGE_ONE_SCENE)):
            e.reset_obs(stages=_stages() | extra)
        for step, a in enumerate((None,) + acts):
            if a is not None:
                for e, extra in zip(envs, (0, L.STAGE_ONE_SCENE)):
                    e.step(torch.from_numpy(a[rows]).to(e.device), stages=_stages() | extra)
            torch.cuda.synchronize()
            for k in ('lidar', 'action_mask', 'status', 'done', 'pose', 'reward', 'reward_info', 'target'):
                u, v = getattr(envs[0], k).cpu().numpy(), getattr(envs[1], k).cpu().numpy()
                assert np.array_equal(u, v), (step, k) + _mismatches(lots, u, v, k)
            for u, v in zip(envs[0].download_state(), envs[1].download_state()):
                assert np.array_equal(u, v), step
        _check(envs[1], lots[:len(rows)], {k: v[rows] for k, v in ref[2].items()}, 'one-scene kernels')
        for e in envs:
            e.close()
    finally:
        os.environ.pop('HOPE_SPLIT_MIN', None)


@pytest.mark.parametrize('form', list(FORMS))
def test_back_face_cull_changes_no_bit_on_adversarial_lots(form):
    """cull on == STAGE_NO_CULL on every family: vertices on beams, thin and undecisive front edges, clockwise, non-convex and sliver
    rings within range"""
    from hope_amd import _lib as L
    lots, sc, acts, ref = reference()
    os.environ['HOPE_SPLIT_MIN'] = FORMS[form][0]
    try:
        envs = [_env(sc, large=FORMS[form][1]) for _ in range(2)]
        for e, extra in zip(envs, (0, L.STAGE_NO_CULL)):
            e.reset_obs(stages=_stages() | extra)
        for step, a in enumerate((None,) + acts):
            if a is not None:
                for e, extra in zip(envs, (0, L.STAGE_NO_CULL)):
                    e.step(torch.from_numpy(a).to(e.device), stages=_stages() | extra)
            torch.cuda.synchronize()
            for k in ('lidar', 'action_mask', 'status', 'pose', 'reward'):
                u, v = getattr(envs[0], k).cpu().numpy(), getattr(envs[1], k).cpu().numpy()
                assert np.array_equal(u, v), (form, step, k) + _mismatches(lots, u, v, k)
        _check(envs[1], lots, ref[2], (form, 'cull off'))
        for e in envs:
            e.close()
    finally:
        os.environ.pop('HOPE_SPLIT_MIN', None)


@pytest.mark.parametrize('form', ['one_launch', 'two_launch_pair_kernels'])
def test_turnover_onto_adversarial_lots(form):
    """every episode ends in one step (time limit) and draws a new lot from a pool of these lots inside the step (auto_reset, fresh):
    the new episode's first scan -- shape flags made at turnover -- and the zero-action step after it equal the oracle's on the
    lots drawn"""
    lots, sc, acts, ref = reference()
    n = len(lots)
    os.environ['HOPE_SPLIT_MIN'] = FORMS[form][0]
    try:
        env = _env(sc)
        env.set_pool(tuple(sc[k] for k in ('start', 'dest', 'bbox', 'verts', 'nob', 'nvert')))
        env.set_redraw_seed(11)
        env.reset_obs(stages=_stages())
        env.upload_state(t=np.full(n, 200, np.int32))
        env.step(torch.from_numpy(acts[0]).to(env.device), stages=_stages(), auto_reset=True, fresh=True)
        torch.cuda.synchronize()
        assert env.done.cpu().numpy().all()
        idx = env.pool_index()
        assert (idx >= 0).all() and env.pool_overflow() == 0
        drawn = [lots[i] for i in idx]
        pose, t, _acc = env.download_state()
        assert np.array_equal(pose, sc['start'][idx]) and (t == 1).all()
        for k in ('lidar', 'action_mask'):
            got, want = getattr(env, k).cpu().numpy(), ref[0][k][idx]
            assert np.array_equal(got, want), (form, 'first scan', k) + _mismatches(drawn, got, want, k)
        env.step(torch.from_numpy(acts[0]).to(env.device), stages=_stages())
        _check(env, drawn, {k: v[idx] for k, v in ref[1].items()}, (form, 'step after turnover'))
        fams = np.bincount([l.fam for l in drawn], minlength=8)
        print(f'turnover ({form}): lots drawn {len(set(idx.tolist()))} of {n}, per family {fams[1:].tolist()}')
        assert (fams[1:] >= 8).all()
        env.close()
    finally:
        os.environ.pop('HOPE_SPLIT_MIN', None)


def test_float32_observations_are_the_rounded_float64_ones():
    """float32 mode stores (float) of the float64 value: lidar, and the mask, equal oracle.astype(float32) exactly"""
    lots, sc, acts, ref = reference()
    env = _env(sc, dtype=torch.float32)
    _run(env, lots, acts, ref, 'float32', cast=np.float32)
    env.close()


@functools.lru_cache(maxsize=None)
def reference_255():
    rng = np.random.default_rng(255)
    lots = [A.lot_255(rng, kept) for kept in (255, 255, 131, 193, 255)]
    sc = A.arrays(lots, 255)
    for l in lots:
        assert A.census(l)['n_kept'] == l.tag[1]
    orc = _oracle(sc, 255)
    ref = [_snap(orc, orc.reset_obs(with_rs=False))]
    zero = np.zeros((len(lots), 2))
    move = np.random.default_rng(256).uniform(-0.5, 0.5, (len(lots), 2))
    ref.append(_snap(orc, orc.step(zero, with_rs=False)))
    ref.append(_snap(orc, orc.step(move, with_rs=False)))
    return lots, sc, (zero, move), ref


@pytest.mark.parametrize('form', ['one_launch', 'two_launch_pair_kernels'])
def test_handle_of_255_obstacles_all_kept(form):
    """max_obstacles = 255 and lots of 255 obstacles, all (or half) of them within range: four chunks of the transform, ring-keep and
    pass-1 loops, the last one partly filled"""
    lots, sc, acts, ref = reference_255()
    os.environ['HOPE_SPLIT_MIN'] = FORMS[form][0]
    try:
        env = _env(sc, mo=255)
        _run(env, lots, acts, ref, (form, '255 obstacles'))
        env.close()
    finally:
        os.environ.pop('HOPE_SPLIT_MIN', None)
