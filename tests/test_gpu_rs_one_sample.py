"""-m gpu: the Reeds-Shepp validation (k_rs_validate_f, k_rs_validate, k_rs_screen + the walk) on the adversarial scenes of
tests/rs_one_sample.py against the CPU oracle (hope_math build, the reference's trailing pop), tolerance 0.0.

 (a) one colliding sample (or two adjacent ones) per word, placed by the restated pass schedule: a walk that drops a sample --
     a wrong index in a coarse or rest round, a lost carried tail, the final sample, the first-segment cache -- finds a word the
     oracle does not;
 (b) diamonds on the goal hull where the reference pops the word's last sample: the kernels must not test it either;
 (c) squares and walls at the float32 filter's margins: same results, and in self-check mode no float32 verdict that the float64
     arithmetic contradicts, while every reason to hesitate and both decided and float64 passes occur.

Handles as in tests/test_gpu_rs_degenerate.py: max_obst = 32 (one tile class) and 128 (both classes, alternating by scene and by
validation form), reset_obs and one zero-action step.
"""
import os

import numpy as np
import pytest

import rs_one_sample as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from test_gpu_rs_degenerate import FORMS, make_env          # noqa: E402

_ref = {}


def reference(max_obst):
    """packed cases and the oracle's reset_obs outputs for them, computed once per obstacle capacity and left unchanged"""
    if max_obst not in _ref:
        from oracle import oracle as O
        from hope_amd import tables as T
        lat = R.build(max_obst)
        n = lat['n']
        t = T.all_tables()
        O.set_tables(hull_base=t['hull_base'], beam_a=t['beam_ab'][:, 0], beam_b=t['beam_ab'][:, 1], dist_star=t['dist_star'], omp=True)
        orc = O.BatchOracle(n, max_obst, omp=True, track_traj=False)
        orc.set_scenes(np.arange(n), lat['start'], lat['dest'], lat['bbox'], lat['verts'], lat['nvert'], lat['n_obst'])
        orc.t[:] = lat['t'] - 1                          # the step increments t before the gate reads it
        o = {k: v.copy() for k, v in orc.reset_obs(with_rs=True).items()}
        _ref[max_obst] = (lat, o)
    return _ref[max_obst]


def check(env, lat, o, tag, ids=None):
    torch.cuda.synchronize()
    ids = np.arange(lat['n']) if ids is None else ids
    w = env.rs_word.cpu().numpy()
    ln = env.rs_lengths.cpu().numpy()
    st = env.status.cpu().numpy()
    bad = np.nonzero((w[:, 6] != o['rs_found'][ids]) | (w[:, :5] != o['rs_ctypes'][ids]).any(axis=1)
                     | (ln != o['rs_lengths'][ids]).any(axis=1) | (st != o['status'][ids]))[0]
    fam = lat['family'][ids]
    print(f'rs_one_sample {tag}: {len(ids)} scenes, found {int((w[:, 6] > 0).sum())}, mismatches {len(bad)}',
          {f: int((fam[bad] == f).sum()) for f in 'abc'}, bad[:20].tolist())
    for i in bad[:5]:
        k = ids[i]
        print('  ', k, fam[i], lat['start'][k].tolist(), lat['dest'][k].tolist(), 'gpu', int(st[i]), w[i].tolist(), ln[i].tolist(),
              'oracle', int(o['status'][k]), int(o['rs_found'][k]), o['rs_ctypes'][k].tolist(), o['rs_lengths'][k].tolist())
    assert len(bad) == 0                                 # tolerance 0.0: status, found flag, types, lengths
    return w, ln


def premises(lat, o):
    """the scenes are searched and both outcomes occur in every family (sample-0 diamonds of family (a) collide with the car at
    the start: the step's gate does not search them, on either side)"""
    searched = o['status'] == 1
    for f, lo, share in (('a', 1500, (0.1, 0.9)), ('b', 400, (0.5, 0.99)), ('c', 1500, (0.1, 0.9))):
        m = lat['family'] == f
        assert (searched & m).sum() > lo, f
        assert share[0] < o['rs_found'][searched & m].mean() < share[1], f


@pytest.mark.parametrize('max_obst', [32, 128])
def test_reset_obs_equals_the_oracle_under_every_validation_form(max_obst):
    from hope_amd import _lib as L
    lat, o = reference(max_obst)
    premises(lat, o)
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
                for v in var:
                    os.environ.pop(v, None)
                env.close()
    finally:
        os.environ.pop('HOPE_SPLIT_MIN', None)
    for form in FORMS:
        assert np.array_equal(out[form][0], out['f32_filter'][0]) and np.array_equal(out[form][1], out['f32_filter'][1]), form


def test_plain_step_equals_the_oracle():
    """the search as the step kernels queue it: one env.step with zero steering and zero speed from every pose"""
    from oracle import oracle as O
    os.environ['HOPE_SPLIT_MIN'] = '1'
    try:
        for max_obst in (32, 128):
            lat, _ = reference(max_obst)
            n = lat['n']
            orc = O.BatchOracle(n, max_obst, omp=True, track_traj=False)
            orc.set_scenes(np.arange(n), lat['start'], lat['dest'], lat['bbox'], lat['verts'], lat['nvert'], lat['n_obst'])
            orc.t[:] = lat['t'] - 1
            act = np.zeros((n, 2))
            o = orc.step(act, with_rs=True)
            assert np.array_equal(orc.pose, lat['start'])                      # zero speed: the car stays where it is
            env = make_env(lat, max_obst)
            try:
                env.step(torch.from_numpy(act).to(env.device))
                check(env, lat, o, f'env.step max_obst={max_obst}')
            finally:
                env.close()
    finally:
        os.environ.pop('HOPE_SPLIT_MIN', None)


def test_margin_cases_in_self_check_mode():
    """family (c) in the statistics build and in self-check mode (HOPE_RS_DEBUG=0x6000): there every sample is evaluated in float64
    as well and float32 verdicts that the float64 arithmetic contradicts are counted; every word the screen condemned is walked
    anyway and must come out invalid"""
    from hope_amd import _lib as L
    from test_gpu_parity import _rs_filter_stats
    max_obst = 32
    lat, o = reference(max_obst)
    ids = np.nonzero(lat['family'] == 'c')[0]
    sub = {k: (v[ids] if isinstance(v, np.ndarray) and v.shape[:1] == (lat['n'],) else v) for k, v in lat.items()}
    sub['n'] = len(ids)
    try:
        _rs_filter_stats(reset=True)
        # 0x4000: the statistics build as the product decides (float64 only for undecided passes: `exact_passes` counts them);
        # 0x6000: self-check of every sample on top (the float64 verdict then decides every pass)
        for mode in ('0x4000', '0x6000'):
            env = make_env(sub, max_obst)
            os.environ['HOPE_RS_DEBUG'] = mode
            try:
                env.reset_obs(stages=L.STAGE_ALL)
                check(env, lat, o, f'HOPE_RS_DEBUG={mode}, family (c)', ids)
            finally:
                os.environ.pop('HOPE_RS_DEBUG', None)
                env.close()
        st = _rs_filter_stats()
    finally:
        os.environ.pop('HOPE_RS_DEBUG', None)
    print('rs_one_sample float32 filter on family (c):', st)
    assert st['samples'] > 100_000
    assert st['bad_hit'] == 0 and st['bad_clear'] == 0 and st['screen_bad'] == 0
    assert all(v > 0 for v in st['undecided_because'].values()), st['undecided_because']
    assert st['hit_passes'] > 0 and st['exact_passes'] > 0 and st['passes'] > st['hit_passes'] + st['exact_passes']
