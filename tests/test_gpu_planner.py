"""The device-resident planner (include/hope_env.h "replay of found Reeds-Shepp paths") on the MI355X: k_plan equals its host twin
bit for bit, it drives the step loop to the torch planner's actions without stopping the host, and misuse fails loudly."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import planner_script as PS  # noqa: E402

pytestmark = pytest.mark.gpu

LEVELS = ('Normal', 'Complex', 'Extrem')
LOT_SEED, BANK_SEED = 7, 1
N_LOTS, N_LOOP_STEPS = 512, 48


@pytest.fixture(scope='module')
def script():
    return PS.make_script()


@pytest.mark.parametrize('obs_dtype', [torch.float32, torch.float64])
def test_kernel_equals_the_host_twin_bit_for_bit(script, obs_dtype):
    """a) the scripted sequence on a 193-scene handle (three full waves and one lane): every output and the state, for float32 and
    float64 lengths and both action types"""
    from hope_amd import ParkingBatch
    from hope_amd import _lib as L
    T, n = script['done'].shape
    assert n == 193
    env = ParkingBatch(n, 32, obs_dtype=obs_dtype)
    env.enable_planner(PS.STEP_RATIO)
    ldt = np.float64 if obs_dtype == torch.float64 else np.float32
    hp = PS.HostPlanner(n)
    dev = env.device
    n_exec = 0
    for t in range(T):
        word = script['word'][t]
        lens = np.ascontiguousarray(script['lengths'][t].astype(ldt))
        done = script['done'][t]
        forced = bool(script['forced'][t])
        adt = (np.float32, np.float64)[t % 2]             # the action types alternate over the steps
        base = np.ascontiguousarray(script['base'][t].astype(adt))
        want_a = base.copy()
        want_p, want_e = hp.step(word, lens, done, L.PLAN_FORCED if forced else 0, want_a)
        act = torch.from_numpy(base).to(dev)
        planned, ex = env.planner_step(forced=forced, step=0, actions=act, rs_word=torch.from_numpy(word).to(dev),
                                       rs_lengths=torch.from_numpy(lens).to(dev), done=torch.from_numpy(done).to(dev))
        assert ex.dtype == torch.bool
        assert np.array_equal(ex.cpu().numpy(), want_e.astype(bool)), t
        assert np.array_equal(planned.cpu().numpy().view(np.uint64), want_p.view(np.uint64)), t
        assert np.array_equal(act.cpu().numpy(), want_a), (t, adt)
        assert np.array_equal(env.planner_state(), hp.state), t
        n_exec += int(want_e.sum())
    assert n_exec > 500
    # reset of some, then of all
    mask = torch.from_numpy((np.arange(n) % 3 == 0).astype(np.uint8)).to(dev)
    busy_before = hp.busy.copy()
    assert busy_before.any()
    env.planner_reset(mask)
    hp.state[:, np.arange(n) % 3 == 0] = 0
    assert np.array_equal(env.planner_state(), hp.state)
    env.planner_reset()
    assert not env.planner_state().any()
    env.close()


def _loop_env(arrs):
    from hope_amd import ParkingBatch
    env = ParkingBatch(N_LOTS, 32, obs_dtype=torch.float64, action_dtype=torch.float64)
    env.set_scene_arrays(np.arange(N_LOTS), *arrs[:5])
    return env


def test_device_planner_inside_the_step_loop_equals_the_torch_planner():
    """b) 512 generated lots, float64, fused turnover, deferred search, 48 steps of a seeded action bank: the device planner (one
    planner_step(step=last_step()) per step, nothing read back until the end) against agent_glue.BatchedRsPlanner on a second
    handle.  The same bank on the CPU oracle env with the torch planner (lot seed 7, bank seed 1) has 141 scenes adopt a
    path and 121 replay one to its end; the floors asserted here are the issue's: 8 and 1."""
    from hope_amd.agent_glue import BatchedRsPlanner
    from hope_amd.scene_gen import mixed_arrays
    arrs = mixed_arrays(N_LOTS, levels=LEVELS, seed=LOT_SEED, max_obst=32)
    bank = torch.from_numpy(np.random.default_rng(BANK_SEED).uniform(-1, 1, (N_LOOP_STEPS, N_LOTS, 2)))
    a, b = _loop_env(arrs), _loop_env(arrs)
    dev = a.device
    bank = bank.to(dev)
    a.enable_planner()
    pl = BatchedRsPlanner(N_LOTS, device=dev)
    a.reset_obs()
    b.reset_obs()
    ex_a, act_a, ex_b, act_b = [], [], [], []
    adopted = torch.zeros(N_LOTS, dtype=torch.bool, device=dev)
    finished = torch.zeros(N_LOTS, dtype=torch.bool, device=dev)
    for t in range(N_LOOP_STEPS):
        # device planner: waits for the search of the last step on the device, overrides the executing rows in place
        act = bank[t].clone()
        _, ex = a.planner_step(step=a.last_step(), actions=act)
        ex_a.append(ex.clone())
        act_a.append(act)
        a.step(act, auto_reset=True, defer_rs=True)
        # torch planner, in HopeRollout._plan's order
        b.wait_rs(step=b.last_step())
        pl.reset(b.done.bool())
        adopted |= pl.set_paths(b.rs_word, b.rs_lengths)
        planned, exb = pl.get_actions()
        finished |= exb & ~pl.executing
        actb = torch.where(exb.unsqueeze(1), planned, bank[t]).contiguous()
        ex_b.append(exb)
        act_b.append(actb)
        b.step(actb, auto_reset=True, defer_rs=True)
    ex_a, act_a, ex_b, act_b = torch.stack(ex_a), torch.stack(act_a), torch.stack(ex_b), torch.stack(act_b)
    n_adopted, n_finished = int(adopted.sum()), int(finished.sum())
    print(f'adopted scenes {n_adopted}, replayed to the end {n_finished}, executing scene-steps {int(ex_b.sum())}')
    assert n_adopted >= 8 and n_finished >= 1
    assert torch.equal(ex_a, ex_b)
    assert torch.equal(act_a, act_b)
    for name in ('pose', 'reward', 'status', 'rs_word', 'rs_lengths'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    a.close()
    b.close()


def test_misuse_fails_loudly_and_off_means_off():
    """c) step before enable, stale step, NULL words; enable + disable leaves a plain step's outputs as on a handle that never did"""
    from hope_amd import ParkingBatch
    from hope_amd import _lib as L
    from hope_amd.scene_gen import mixed_arrays
    n = 64
    arrs = mixed_arrays(n, levels=LEVELS, seed=3, max_obst=32)
    envs = [ParkingBatch(n, 32, obs_dtype=torch.float64, action_dtype=torch.float64) for _ in range(2)]
    for e in envs:
        e.set_scene_arrays(np.arange(n), *arrs[:5])
        e.reset_obs()
    env, plain = envs
    lib = env.lib
    planned = torch.zeros((n, 2), dtype=torch.float64, device=env.device)
    ex = torch.zeros(n, dtype=torch.uint8, device=env.device)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def raw_step(word=True, lens=True, step=0):
        return lib.hope_env_planner_step(env.h, P(env.rs_word) if word else None, P(env.rs_lengths) if lens else None, P(env.done), 0,
                                         C.c_uint64(step), P(planned), P(ex), None, 0, env._stream())
    assert raw_step() == -5 and b'planner is off' in lib.hope_last_error()             # HOPE_ESTATE
    assert lib.hope_env_planner_reset(env.h, None, env._stream()) == -5
    with pytest.raises(L.HopeError):
        env.planner_step()
    env.enable_planner()
    assert raw_step(word=False) == -1 and raw_step(lens=False) == -1                   # HOPE_EINVAL
    old = env.last_step()
    assert raw_step(step=old) == 0
    act = torch.zeros((n, 2), dtype=torch.float64, device=env.device)
    for e in envs:
        e.step(act, defer_rs=True)
    assert raw_step(step=old) == -5 and b'not the last one' in lib.hope_last_error()   # a newer step replaced its words
    assert raw_step(step=env.last_step() + 1) == -1
    assert raw_step(step=env.last_step()) == 0
    assert lib.hope_env_planner_step(env.h, P(env.rs_word), P(env.rs_lengths), None, 4, C.c_uint64(0), None, None, None, 0, env._stream()) == -1
    env.disable_planner()
    assert raw_step() == -5
    rng = np.random.default_rng(0)
    for _ in range(3):
        act = torch.from_numpy(rng.uniform(-1, 1, (n, 2))).to(env.device)
        for e in envs:
            e.step(act, auto_reset=True)
    torch.cuda.synchronize()
    for name in ('lidar', 'action_mask', 'target', 'reward', 'reward_info', 'status', 'done', 'pose', 'rs_word', 'rs_lengths'):
        assert torch.equal(getattr(env, name), getattr(plain, name)), name
    for e in envs:
        e.close()
