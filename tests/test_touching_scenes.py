"""The premise of the touching-scene tests of tests/test_gpu_exact_geometry.py, checked without a GPU: the scenes that
tests/touching_scenes.py builds do reach the collision test's robust path -- "undecided by the orientation filter, no certain
hit" at a pose the reference's step visits -- on at least a quarter of the adversarial scenes, with each exact answer at least a
tenth of those, and the oracle gives the exact answer there.  Same seeds and sizes as the GPU tests."""
import numpy as np
import pytest

import touching_scenes as T
from oracle import oracle as O

CONTINUE, COLLIDED = 1, 3


@pytest.mark.parametrize('case', ['static', 'moving', 'pool'])
def test_touching_scenes_reach_the_robust_path_with_both_answers(case):
    n = 600 if case == 'pool' else 1501
    sc = T.build(n, {'static': 41, 'moving': 42, 'pool': 43}[case], case == 'moving', layout='alternate' if case == 'pool' else 'mixed',
                 dest_near=case == 'pool')
    assert sc['nob'].max() <= 32 and sc['adv'].sum() >= n // 2
    if case != 'pool':
        assert sc['adv'][:n // 3].all() and not sc['adv'][n // 3 + 1::2].any()       # consecutive ids, then in turn with plain scenes
    for i in np.nonzero(sc['many'])[0]:
        poses = np.vstack([sc['start'][i][None], T.substep_poses(sc['start'][i], sc['action'][i])])
        assert 9 <= T.near_count(poses, sc['verts'][i, :sc['nob'][i]]) <= 12
    robust, answer = T.assert_premise(sc, reset=case != 'moving', tag=case)
    if case == 'moving':
        assert len(np.unique(sc['kstar'][robust])) == 10
        return
    # the start pose's status in the oracle is the exact answer wherever the robust path decides it
    orc = O.BatchOracle(n, 128, track_traj=False)
    orc.set_scenes(np.arange(n), sc['start'], sc['dest'], sc['bbox'], sc['verts'], sc['nvert'], sc['nob'])
    st = orc.reset_obs(with_rs=False)['status']
    assert (st[robust & (answer == 1)] == COLLIDED).all() and (st[robust & (answer == 0)] != COLLIDED).all()
    if case == 'pool':                                            # the first reward term tells the two answers apart
        assert (orc.accum[robust & (answer == 0)] > 0).all() and (orc.accum[robust & (answer == 1)] == 0).all()
    T.assert_premise(sc, reset=False, tag=case + ', zero-action step')
