"""k_choose (hope_amd/csrc/hope_chooser_kernel.h) on the device: bit-equal to its host twin, inside a real step loop, and misused."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chooser_script as CS  # noqa: E402

pytestmark = pytest.mark.gpu

N, CALLS = 193, 20                                                 # three full waves and one lane


def _np(dt):
    return np.float64 if dt == torch.float64 else np.float32


def _views_equal(got, want, what):
    got = np.ascontiguousarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype)
    v = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    assert np.array_equal(got.view(v), np.ascontiguousarray(want).view(v)), what


def _call_both(env, mean, log_std, mask, planned, executing, u, seed, counter, probs, what):
    """one choose_actions call and the host twin on the same arrays; every output compared as raw words"""
    dev = env.device
    D = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    out = env.choose_actions(D(mean), D(log_std), D(mask), D(planned), D(executing), D(u), seed, counter, probs=probs)
    want = CS.host_choose(mean, log_std, mask, planned, executing, u, seed, counter, 0, env.action_dtype == torch.float64, probs)
    names = ('action', 'action_f32', 'idx', 'log_prob') + (('probs',) if probs else ())
    assert len(out) == len(names)
    got = {k: t.cpu().numpy() for k, t in zip(names, out)}
    for k in names:
        _views_equal(got[k], want[k], (what, k))
    assert out[0].dtype == env.action_dtype and out[0].is_contiguous() and out[0].shape == (env.n, 2)
    return got


@pytest.fixture(scope='module')
def rows():
    mean, log_std, mask, u = CS.random_rows(N * CALLS)
    pl = np.random.default_rng(2)
    planned = np.stack([pl.integers(-1, 2, N * CALLS).astype(np.float64), pl.uniform(-1, 1, N * CALLS)], axis=1)
    executing = (pl.random(N * CALLS) < 0.25).astype(np.uint8)
    return mean, log_std, mask, u, planned, executing, CS.edge_rows()


@pytest.mark.parametrize('action_dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('obs_dtype', [torch.float32, torch.float64])
def test_kernel_equals_the_host_twin_bit_for_bit(rows, obs_dtype, action_dtype):
    """a) 193 scenes, obs_dtype x action_dtype: the random rows in 20 calls that alternate float32 / float64 inputs, broadcast /
    per-row log_std, supplied / counter-based u, with / without planned + executing, with / without probs; then the edge rows
    (checked against their hand-computed expectations as well); every output equals the twin's as raw words"""
    from hope_amd import ParkingBatch
    mean, log_std, mask, u, planned, executing, (edge, want) = rows
    env = ParkingBatch(N, 32, obs_dtype=obs_dtype, action_dtype=action_dtype)
    env.enable_chooser()
    mdt = _np(obs_dtype)
    for t in range(CALLS):
        s = slice(t * N, (t + 1) * N)
        idt = (np.float32, np.float64)[t & 1]
        ls = log_std[s][:1] if (t >> 1) & 1 else log_std[s]
        with_u, with_plan, with_probs = t % 3 != 2, t % 4 < 2, t % 5 != 4
        _call_both(env, mean[s].astype(idt), ls.astype(idt), mask[s].astype(mdt), planned[s] if with_plan else None,
                   executing[s] if with_plan else None, u[s] if with_u else None, 77, t, with_probs, t)
    # the outputs are persistent tensors of the object; a float32 env steps with the tensor the ring stores
    a, a32, _, _ = env.choose_actions(torch.zeros((N, 2), device=env.device), torch.zeros((1, 2), device=env.device),
                                      torch.ones((N, 42), dtype=obs_dtype, device=env.device))
    assert a is env.chosen_action and a32 is env.chosen_action_f32 and (a is a32) == (action_dtype == torch.float32)
    ne = len(edge['u'])
    assert ne <= N
    pad = lambda e, r: np.concatenate([e, r[:N - ne]])  # noqa: E731
    for idt in (np.float32, np.float64):
        got = _call_both(env, pad(edge['mean'], mean).astype(idt), pad(edge['log_std'], log_std).astype(idt), pad(edge['mask'], mask).astype(mdt),
                         pad(edge['planned'], planned), pad(edge['executing'], executing * 0), pad(edge['u'], u), 0, 0, True, ('edge', idt))
        CS.check_edge_rows(edge, want, {k: v[:ne] for k, v in got.items()})
    env.close()


@pytest.mark.parametrize('n', [1, 64])
def test_one_scene_and_one_full_wave(rows, n):
    from hope_amd import ParkingBatch
    mean, log_std, mask, u, planned, executing, _ = rows
    env = ParkingBatch(n, 32, obs_dtype=torch.float64, action_dtype=torch.float32)
    env.enable_chooser()
    s = slice(300, 300 + n)
    _call_both(env, mean[s], log_std[s].astype(np.float32), mask[s], planned[s], executing[s], u[s], 0, 0, True, n)
    _call_both(env, mean[s].astype(np.float64), log_std[s][:1], mask[s], None, None, None, 5, 9, False, n)
    env.close()


def test_chooser_inside_the_step_loop_equals_the_torch_path():
    """b) 512 generated lots (mixed_arrays, seed 7, max_obst 32), float64, fused turnover, deferred search, device planner,
    StandInPolicy, 24 steps: planner_step(step=last_step()) -> choose_actions(supplied u bank, probs) -> step(the device's action
    tensor).  Per step torch's mask_action_probs and a cumsum pick on the same inputs; nothing is read back inside the loop.
    Indices equal outside the 1e-9 band (at most 0.1 % of the rows in it), probs within 1e-12 relative, executing rows carry
    (float32) planned, the others a row of the action table.
    The floor: `python tests/chooser_script.py` -- the same loop on the CPU oracle env (float32 observations, host twins of planner
    and chooser) -- has 132 scenes replay a planned action in 1857 scene-steps.  The float64 device env follows other trajectories
    (its policy sees other last bits), so the floor asserted is a quarter of that: 33 scenes and 464 scene-steps -- enough to say that
    the override was exercised, far enough from 132 / 1857 that only a broken search or planner hand-over can miss it."""
    from hope_amd import ParkingBatch
    from hope_amd.rollout import StandInPolicy
    arrs = CS.loop_arrays()
    env = ParkingBatch(CS.LOOP_LOTS, 32, obs_dtype=torch.float64, action_dtype=torch.float64)
    env.set_scene_arrays(np.arange(CS.LOOP_LOTS), *arrs[:5])
    env.enable_planner()
    env.enable_chooser()
    env.reset_obs()
    dev = env.device
    torch.manual_seed(0)
    policy = StandInPolicy().to(dev).eval()
    u_bank = torch.from_numpy(np.random.default_rng(CS.LOOP_U_SEED).random((CS.LOOP_STEPS, CS.LOOP_LOTS))).to(dev)

    def plan():
        return env.planner_step(step=env.last_step())

    def choose(mean, log_std, planned, ex, u):
        a, _, idx, _, probs = env.choose_actions(mean, log_std, None, planned, ex, u, probs=True)
        return a, idx, probs
    acc = CS.step_loop(env, policy, plan, choose, u_bank, {'defer_rs': True})
    got = {k: (int(v.sum()) if v.dtype != torch.float64 else float(v)) for k, v in acc.items()}        # the one read-back
    print(got)
    assert got['rows'] == CS.LOOP_LOTS * CS.LOOP_STEPS
    assert got['near'] + got['flagged'] <= got['rows'] // 1000
    assert got['idx_diff'] == 0 and got['support_diff'] == 0
    assert got['max_rel'] <= 1e-12
    assert got['exec_wrong'] == 0 and got['table_wrong'] == 0
    assert got['exec_scenes'] >= 33 and got['exec_steps'] >= 464
    env.close()


def test_misuse_fails_loudly():
    """c) choose before enable (HOPE_ESTATE), planned without executing and the reverse, wrong dtype / shape / layout, NULL required
    pointers (assertion or HOPE_EINVAL); disable and enable again works"""
    from hope_amd import ParkingBatch
    from hope_amd import _lib as L
    n = 70
    env = ParkingBatch(n, 32)
    dev, lib = env.device, env.lib
    mean = torch.zeros((n, 2), device=dev)
    ls = torch.zeros((1, 2), device=dev)
    mask = torch.ones((n, 42), device=dev)
    planned = torch.zeros((n, 2), dtype=torch.float64, device=dev)
    ex = torch.zeros(n, dtype=torch.uint8, device=dev)
    act = torch.zeros((n, 2), device=dev)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731

    def raw(mean=mean, ls=ls, stride=0, mask=mask, planned=None, executing=None, action=act):
        return lib.hope_env_choose(env.h, P(mean), P(ls), stride, 0, P(mask), P(planned), P(executing), None, 0, 0, P(action), None, None, None, None,
                                   env._stream())
    assert raw() == -5 and b'chooser is off' in lib.hope_last_error()                   # HOPE_ESTATE
    with pytest.raises(L.HopeError, match='code -5'):
        env.choose_actions(mean, ls, mask)
    env.enable_chooser()
    assert raw() == 0
    assert raw(planned=planned, executing=ex) == 0
    for kw in ({'mean': None}, {'ls': None}, {'mask': None}, {'action': None}, {'planned': planned}, {'executing': ex}, {'stride': 1}):
        assert raw(**kw) == -1, kw                                                     # HOPE_EINVAL
    assert raw(action=act.view(-1)[1:]) == -1                                          # a misaligned action row
    bad = [dict(mean=mean.double()), dict(mean=mean[:-1]), dict(mean=torch.zeros((2, n), device=dev).t()), dict(log_std=torch.zeros((2, 2), device=dev)),
           dict(mask=mask.double()), dict(mask=mask[:, :41]), dict(planned=planned), dict(executing=ex), dict(planned=planned.float(), executing=ex),
           dict(planned=planned, executing=ex[:-1]), dict(u=torch.zeros(n, device=dev)), dict(mean=mean.cpu())]
    for kw in bad:
        args = dict(mean=mean, log_std=ls, mask=mask)
        args.update(kw)
        with pytest.raises(L.HopeError):
            env.choose_actions(**args)
    bad_table = CS.ACTS.copy()
    bad_table[30, 0] += 0.01
    assert lib.hope_env_chooser_enable(env.h, bad_table.ctypes.data) == -1 and lib.hope_env_chooser_enable(env.h, None) == -1
    first = [t.clone() for t in env.choose_actions(mean, ls, mask, seed=3, counter=4)]
    env.disable_chooser()
    assert raw() == -5
    with pytest.raises(L.HopeError, match='code -5'):
        env.choose_actions(mean, ls, mask)
    env.enable_chooser()
    again = env.choose_actions(mean, ls, mask, seed=3, counter=4)
    assert all(torch.equal(x, y) for x, y in zip(first, again))
    env.disable_chooser()
    env.disable_chooser()                                                              # (idempotent, like the planner's)
    env.close()
