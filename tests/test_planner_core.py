"""The path-replay rule of hope_amd/csrc/hope_planner_core.h through its host twin hope_planner_step_host: against the
reference's own action lists (tests/golden/agent_glue.npz, tests/golden/rs_planner_quirks.npz), against the torch class's
sequence semantics, and inside the rollout loop on the CPU stand-in env."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import planner_script as PS  # noqa: E402


def _check_fixture(g):
    off = g['action_off']
    got = PS.expand_all(g['words'], g['lengths'])
    assert len(got) == len(off) - 1
    for i, a in enumerate(got):
        want = g['actions'][off[i]:off[i + 1]]
        assert a.shape == want.shape, (i, a.shape, want.shape)
        assert np.array_equal(a.view(np.uint64), np.ascontiguousarray(want).view(np.uint64)) or np.array_equal(a, want), i
    return got


def test_host_twin_reproduces_the_reference_action_lists_without_a_cap(gold):
    """a) RsPlanner.set_rs_path's lists of the existing fixture -- raw calc_all_paths words, some hundreds of metres long"""
    g = gold('agent_glue.npz')
    got = _check_fixture(g)
    assert max(len(a) for a in got) > 96                 # (longer than the torch class's queue)


def test_host_twin_reproduces_the_reference_on_the_edges_of_the_rule(gold):
    """b) one step exactly, integer step counts, one ulp around them, the 1e-3 keep threshold, +-0, float32-rounded copies"""
    g = gold('rs_planner_quirks.npz')
    _check_fixture(g)
    # rows whose lengths are float32 numbers give the same lists through the float32 input path
    l32 = g['lengths'].astype(np.float32)
    rows = np.nonzero((l32.astype(np.float64) == g['lengths']).all(1))[0]
    assert len(rows) >= len(g['lengths']) // 4
    off = g['action_off']
    got = PS.expand_all(g['words'][rows], l32[rows])
    for k, i in enumerate(rows):
        assert np.array_equal(got[k], g['actions'][off[i]:off[i + 1]]), i


def test_non_finite_lengths_and_bad_arguments():
    hp = PS.HostPlanner(3)
    word = np.zeros((3, 8), np.int8)
    word[:, :5] = [1, 0, 2, -1, -1]
    word[:, 5], word[:, 6] = 3, 1
    lens = np.zeros((3, 5))
    lens[0, :3] = [np.inf, 0.5, np.nan]                  # only the middle segment contributes
    lens[1, :3] = [np.nan, -np.inf, np.inf]              # nothing: stays idle
    lens[2, :3] = [1e300, 0.0, 0.0]                      # k clamps to 2^31 - 1: replay starts, no overflow
    planned, ex = hp.step(word, lens)
    assert ex.tolist() == [1, 0, 1] and planned[0].tolist() == [0.0, 0.4] and planned[1].tolist() == [0.0, 0.0]
    assert planned[2].tolist() == [1.0, 1.0] and hp.busy.tolist() == [False, False, True]
    from hope_amd import _lib as L
    lib = L.load_library()
    st = np.zeros((6, 3), np.uint64)
    assert lib.hope_planner_step_host(3, 1.25, st.ctypes.data, None, lens.ctypes.data, 1, None, 0, None, None, None, 0) == -1
    assert lib.hope_planner_step_host(3, 1.25, st.ctypes.data, word.ctypes.data, None, 1, None, 0, None, None, None, 0) == -1
    assert lib.hope_planner_step_host(0, 1.25, st.ctypes.data, word.ctypes.data, lens.ctypes.data, 1, None, 0, None, None, None, 0) == -1
    assert lib.hope_planner_step_host(3, -1.0, st.ctypes.data, word.ctypes.data, lens.ctypes.data, 1, None, 0, None, None, None, 0) == -1


@pytest.fixture(scope='module')
def script():
    return PS.make_script()


@pytest.mark.parametrize('ldt', [np.float64, np.float32])
def test_sequence_semantics_equal_the_torch_planner(script, ldt):
    """c) 193 scenes x 60 scripted steps: offers while busy, episode ends in mid-replay, forced adoption every seventh step"""
    ex_t, planned_t, (adopted, refused, mid) = PS.torch_reference(script, ldt)
    assert adopted >= 50 and refused >= 10 and mid >= 10, (adopted, refused, mid)
    L = PS.HostPlanner(1).L
    T, n = script['done'].shape
    hp = PS.HostPlanner(n)
    for t in range(T):
        flags = L.PLAN_FORCED if script['forced'][t] else 0
        a32 = np.ascontiguousarray(script['base'][t].astype(np.float32))
        a64 = script['base'][t].copy()
        keep = hp.state.copy()
        planned, ex = hp.step(script['word'][t], script['lengths'][t].astype(ldt), script['done'][t], flags, a32)
        hp.state[:] = keep                                # the same step once more for the float64 action buffer
        planned2, ex2 = hp.step(script['word'][t], script['lengths'][t].astype(ldt), script['done'][t], flags, a64)
        assert np.array_equal(planned, planned2) and np.array_equal(ex, ex2)
        e = ex_t[t]
        assert np.array_equal(ex.astype(bool), e), t
        assert np.array_equal(planned[e], planned_t[t][e]), t
        assert (planned[~e] == 0).all()
        base = torch.from_numpy(script['base'][t])
        for got, dt in ((a32, torch.float32), (a64, torch.float64)):
            b = base.to(dt)
            want = torch.where(torch.from_numpy(e).unsqueeze(1), torch.from_numpy(planned_t[t]).to(dt), b)
            assert np.array_equal(got, want.numpy()), (t, dt)
    assert ex_t.sum() > 500


def _small_scenes(n, seed=3):
    from hope_amd.scenes import SceneSource
    src = SceneSource(levels=('Normal', 'Complex', 'Extrem'), seed=seed)
    return [src.draw() for _ in range(n)]


def test_rollout_with_the_device_planner_equals_the_torch_planner_on_the_cpu():
    """d) HopeRollout on the oracle env, use_planner=True vs 'device', same seeds: every action, log-prob and stat over 40 steps"""
    from fake_env import OracleEnv
    from hope_amd import agents as A
    from hope_amd import agent_glue as G
    from hope_amd.rollout import HopeRollout
    scenes = _small_scenes(12)
    runs = []
    for mode in (True, 'device'):
        torch.manual_seed(0)
        env = OracleEnv(scenes)
        ag = A.BatchedPPO(device='cpu', use_img=False, lr=1e-4, mini_batch=24, mini_epoch=2)
        ro = HopeRollout(env, ag, horizon=40, seed=1, use_planner=mode)
        assert isinstance(ro.planner, G.DeviceRsPlanner if mode == 'device' else G.BatchedRsPlanner)
        busy = []
        for _ in range(40):
            ro.collect_step()
            busy.append(ro.planner.executing.numpy().copy())
        runs.append((ro.ring.action.clone(), ro.ring.log_prob.clone(), ro.ring.reward.clone(), ro.ring.done.clone(), ro.stats(), np.array(busy)))
    a, b = runs
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    assert a[4] == b[4]
    assert np.array_equal(a[5], b[5])
    assert a[5].any(axis=0).sum() >= 1                    # (a path was found and replayed: the planners had something to do)


def test_sac_trainer_and_evaluator_take_the_device_planner():
    """use_planner='device' in the SAC loop (random-action phase and policy phase) and in the batched evaluator (frozen slots,
    masked words): the same actions / records as use_planner=True"""
    from fake_env import OracleEnv
    from hope_amd import agents as A
    from hope_amd import evaluate as E
    from hope_amd.rollout import SACTrainer
    scenes = _small_scenes(8, seed=5)
    runs = []
    for mode in (True, 'device'):
        torch.manual_seed(0)
        tr = SACTrainer(OracleEnv(scenes), A.BatchedSAC(device='cpu', use_img=False, lr=1e-4, batch_size=16), horizon=8, update_every=1000,
                        seed=2, use_planner=mode)
        for _ in range(16):
            tr.step()
        runs.append((tr.ring.action.clone(), tr.ring.log_prob.clone(), tr.ring.done.clone(), tr.stats()))
    assert all(torch.equal(x, y) for x, y in zip(runs[0][:3], runs[1][:3])) and runs[0][3] == runs[1][3]
    recs = []
    for mode in (True, 'device'):
        torch.manual_seed(0)
        ev = E.BatchedEvaluator(OracleEnv(scenes), A.BatchedPPO(device='cpu', use_img=False), seed=5, use_planner=mode)
        recs.append(ev.run(max_steps=25, gather=False))
    assert torch.equal(recs[0], recs[1])
    with pytest.raises(ValueError):
        SACTrainer(OracleEnv(scenes[:2]), A.BatchedSAC(device='cpu', use_img=False, batch_size=4), horizon=2, use_planner='gpu')
