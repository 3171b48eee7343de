"""-m gpu: the Reeds-Shepp search chain (k_rs_compact -> k_rs_words -> k_rs_segs -> k_rs_validate_f) on the lattice of exactly
aligned and degenerate poses of tests/rs_degenerate.py against the CPU oracle (hope_math build), tolerance 0.0.

Two handles: max_obst = 32 has one tile class and runs one chain with the one-launch step kernel; max_obst = 128 holds the lattice
in BOTH tile classes (alternate scenes moved to the large-tile class), so that with HOPE_SPLIT_MIN=1 the step runs two chains on two
streams, k_rs_compact fills both class queues, and the step kernel takes its two-launch form with the pair kernels on the small-tile
class (plan_step, hope_env.hip).  The class of a scene alternates from one validation form to the next, so every lattice case runs
in either class.

Words with zero-length segments, solver guards on their boundaries, sample counts that the reference's trailing pop changes, the
10 m / t > 1 gate on 10.0 and its float64 neighbours: every validation form must give the oracle's bits.
"""
import os

import numpy as np
import pytest

import rs_degenerate as D

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

FORMS = {'f32_filter': {}, 'exact': {'HOPE_RS_EXACT': '1'}, 'no_screen': {'HOPE_RS_DEBUG': '0x20000'}, 'split': {'HOPE_RS_SPLIT': '1'}}
_ref = {}


def reference(max_obst):
    """lattice arrays and the oracle's reset_obs outputs for them, computed once per obstacle capacity and left unchanged"""
    if max_obst not in _ref:
        from oracle import oracle as O
        from hope_amd import tables as T
        lat = D.build(max_obst)
        n = lat['n']
        t = T.all_tables()
        O.set_tables(hull_base=t['hull_base'], beam_a=t['beam_ab'][:, 0], beam_b=t['beam_ab'][:, 1], dist_star=t['dist_star'], omp=True)
        orc = O.BatchOracle(n, max_obst, omp=True, track_traj=False)
        orc.set_scenes(np.arange(n), lat['start'], lat['dest'], lat['bbox'], lat['verts'], lat['nvert'], lat['n_obst'])
        orc.t[:] = lat['t'] - 1                          # the step increments t before the gate reads it
        o = {k: v.copy() for k, v in orc.reset_obs(with_rs=True).items()}
        _ref[max_obst] = (lat, o)
    return _ref[max_obst]


def make_env(lat, max_obst, flip=0, profile=False):
    """the lattice in a fresh handle.  max_obst > 32: set_scene_arrays puts every lattice scene (<= 2 obstacles) into the small-tile
    class; the scenes with (id + flip) odd move to the large-tile class, so the handle holds both classes, half the lattice each"""
    from hope_amd import ParkingBatch
    n = lat['n']
    env = ParkingBatch(n, max_obst, obs_dtype=torch.float64, action_dtype=torch.float64, overlap=True, profile=profile)
    try:
        assert env.arch.startswith('gfx950'), env.arch
        env.set_scene_arrays(np.arange(n), lat['start'], lat['dest'], lat['bbox'], lat['verts'], lat['n_obst'])
        if max_obst > 32:
            env.set_draw_class(np.arange((1 + flip) % 2, n, 2), 1)
        env.upload_state(pose=lat['start'], t=lat['t'] - 1)
    except BaseException:
        env.close()
        raise
    return env


def check(env, lat, o, tag):
    torch.cuda.synchronize()
    w = env.rs_word.cpu().numpy()
    ln = env.rs_lengths.cpu().numpy()
    bad = np.nonzero((w[:, 6] != o['rs_found']) | (w[:, :5] != o['rs_ctypes']).any(axis=1) | (ln != o['rs_lengths']).any(axis=1))[0]
    print(f'rs_degenerate {tag}: {lat["n"]} scenes, found {int((w[:, 6] > 0).sum())}, mismatches {len(bad)}', bad[:20].tolist())
    for i in bad[:5]:
        print('  ', i, lat['start'][i].tolist(), lat['dest'][i].tolist(), 'variant', int(lat['variant'][i]), 'gpu', w[i].tolist(),
              ln[i].tolist(), 'oracle', int(o['rs_found'][i]), o['rs_ctypes'][i].tolist(), o['rs_lengths'][i].tolist())
    assert np.array_equal(env.status.cpu().numpy(), o['status'])
    assert len(bad) == 0                                                       # tolerance 0.0: types, found flag, lengths
    # the gate: searched iff d < 10 and t > 1; an unsearched scene has the cleared word
    searched = (lat['gate_d'] < 10.0) & (lat['t'] > 1) & (o['status'] == 1)
    un = ~searched
    assert (w[un, :5] == -1).all() and (w[un, 5:] == 0).all() and (ln[un] == 0).all()
    g = lat['gate']
    assert np.array_equal(w[g, 6] > 0, searched[g]) and searched[g].sum() == 2          # no obstacle there: searched == found
    return w, ln


@pytest.mark.parametrize('max_obst', [32, 128])
def test_reset_obs_equals_the_oracle_under_every_validation_form(max_obst):
    from hope_amd import _lib as L
    lat, o = reference(max_obst)
    assert o['rs_found'].sum() > 2000 and (o['status'] == 1).sum() > 3900      # (3 m ahead, heading reversed: ARRIVED, not searched)
    os.environ['HOPE_SPLIT_MIN'] = '1'
    out = {}
    try:
        for k, (form, var) in enumerate(FORMS.items()):
            env = make_env(lat, max_obst, flip=k % 2)                          # a fresh handle per form, one launch each
            os.environ.update(var)
            try:
                env.reset_obs(stages=L.STAGE_ALL)
                out[form] = check(env, lat, o, f'{form} max_obst={max_obst}')
            finally:
                for k in var:
                    os.environ.pop(k, None)
                env.close()
    finally:
        os.environ.pop('HOPE_SPLIT_MIN', None)
    for form in FORMS:
        assert np.array_equal(out[form][0], out['f32_filter'][0]) and np.array_equal(out[form][1], out['f32_filter'][1]), form


def oracle_step(lat, max_obst):
    from oracle import oracle as O
    n = lat['n']
    orc = O.BatchOracle(n, max_obst, omp=True, track_traj=False)
    orc.set_scenes(np.arange(n), lat['start'], lat['dest'], lat['bbox'], lat['verts'], lat['nvert'], lat['n_obst'])
    orc.t[:] = lat['t'] - 1
    act = np.zeros((n, 2))
    o = orc.step(act, with_rs=True)
    assert np.array_equal(orc.pose, lat['start'])                              # zero speed: the car stays where it is
    return orc, act, o


def test_plain_step_from_the_lattice_equals_the_oracle():
    """the search as the step kernels queue it: one env.step with zero steering and zero speed from every lattice pose.  max_obst =
    128: both tile classes, hence two chains and the two-launch form with k_motion_pair / k_obs_pair on the small-tile class"""
    os.environ['HOPE_SPLIT_MIN'] = '1'
    try:
        for max_obst in (32, 128):
            lat, _ = reference(max_obst)
            orc, act, o = oracle_step(lat, max_obst)
            env = make_env(lat, max_obst)
            try:
                env.step(torch.from_numpy(act).to(env.device))
                check(env, lat, o, f'env.step max_obst={max_obst}')
                pose, t, _ = env.download_state()
                assert np.array_equal(pose, orc.pose) and np.array_equal(t, orc.t.astype(np.int32))
            finally:
                env.close()
    finally:
        os.environ.pop('HOPE_SPLIT_MIN', None)


def test_two_class_handle_runs_two_chains_in_the_two_launch_form():
    """the premise of the max_obst = 128 runs above, read off a handle that counts its launches (profile=True; the plan is the same,
    launch_step): per call one k_rs_compact, one k_rs_words and one validation launch per tile class, and the step kernel launched
    twice per class (motion, observation).  Results as above, with the classes the other way round than in the step test."""
    from hope_amd import _lib as L
    max_obst = 128
    lat, o_reset = reference(max_obst)
    _, act, o_step = oracle_step(lat, max_obst)
    os.environ['HOPE_SPLIT_MIN'] = '1'
    env = None
    try:
        env = make_env(lat, max_obst, flip=1, profile=True)
        env.reset_obs(stages=L.STAGE_ALL)
        check(env, lat, o_reset, 'reset_obs, counted launches')
        km = {k: v[1] for k, v in env.kernel_ms().items()}
        print('rs_degenerate reset_obs launches:', km)
        assert km['k_rs_compact'] == 2 and km['k_rs_words'] == 2 and km['k_rs_validate'] == 2 and km['k_env_step'] == 4
        env.upload_state(pose=lat['start'], t=lat['t'] - 1)
        env.step(torch.from_numpy(act).to(env.device))
        check(env, lat, o_step, 'env.step, counted launches')
        km = {k: v[1] for k, v in env.kernel_ms().items()}
        print('rs_degenerate env.step launches:', km)
        assert km['k_rs_compact'] == 2 and km['k_rs_words'] == 2 and km['k_rs_validate'] == 2 and km['k_env_step'] == 4
        assert km['k_kinematics'] == 2                                         # (not fused into the step kernel: the two-launch form)
    finally:
        os.environ.pop('HOPE_SPLIT_MIN', None)
        if env is not None:
            env.close()
