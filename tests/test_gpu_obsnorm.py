"""k_obsnorm_partial / k_obsnorm_merge / k_obsnorm_apply (hope_amd/csrc/hope_obsnorm_kernel.h) on the device: bit-equal to their host
twin, the statistics' round trip, inside a real step loop next to the torch path, and misused."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import obsnorm_script as OS  # noqa: E402

pytestmark = pytest.mark.gpu


def _same_stats(env, twin, what):
    n, mean, S, std = env.obsnorm_state()
    assert n == twin.n_state == env.obsnorm_count(), what
    for got, want, name in zip((mean, S, std), twin.stats(), ('mean', 'S', 'std')):
        assert np.array_equal(OS.words(got), OS.words(want)), (what, name)


def _call_both(env, twin, lidar, target, update, normalize, what):
    """one obsnorm call and the host twin on the same arrays: statistics and outputs compared as raw words"""
    D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(env.device)  # noqa: E731
    got = env.obsnorm(D(lidar), D(target), update=update, normalize=normalize)
    want = twin(lidar, target, update=update, normalize=normalize)
    _same_stats(env, twin, what)
    if normalize:
        for g, w, name in zip(got, want, ('lidar', 'target')):
            assert g.dtype == torch.float32 and g.shape == w.shape and g.is_contiguous(), (what, name)
            assert np.array_equal(OS.words(g.cpu().numpy()), OS.words(w)), (what, name)
    else:
        assert got == (None, None)


def _zero(env):
    z = np.zeros(OS.NC)
    env.obsnorm_load(0, z, z, z)


@pytest.mark.parametrize('dt', [np.float32, np.float64])
def test_kernels_equal_the_host_twin_bit_for_bit(dt):
    """a handle of 321 scenes; per row count 1, 2, 63, 64, 65, 193, 321: from n_state == 0 an update (alone, or with the
    normalisation), then onto n_state > 0 an update with the normalisation, a normalisation alone and an update alone; mean, S and
    std after every call and both outputs equal the twin's as raw words"""
    from hope_amd import ParkingBatch
    env = ParkingBatch(321, 32)
    env.enable_obsnorm()
    for j, rows in enumerate(OS.ROW_COUNTS):
        _zero(env)
        twin = OS.HostNorm()
        obs = [OS.observations(rows, seed=100 * rows + k, dtype=dt) for k in range(4)]
        _call_both(env, twin, *obs[0], True, bool(j & 1), (rows, 'first'))
        _call_both(env, twin, *obs[1], True, True, (rows, 'both'))
        _call_both(env, twin, *obs[2], False, True, (rows, 'normalize'))
        _call_both(env, twin, *obs[3], True, False, (rows, 'update'))
        assert twin.n_state == 3 * rows
    # the outputs are persistent tensors of the object
    nl, nt = env.obsnorm(update=False)
    assert nl is env.norm_lidar and nt is env.norm_target and nl.shape == (321, 120) and nt.shape == (321, 5)
    env.close()


def test_more_leaves_than_lanes_in_the_merge_wave():
    """a handle of 4 160 scenes: 65 chunks -- more leaves than the merge wave has lanes, with an odd leaf -- from n_state == 0 (the
    last chunk is one row short) and onto n_state > 0, float32 and float64"""
    from hope_amd import ParkingBatch
    env = ParkingBatch(4160, 32)
    env.enable_obsnorm()
    twin = OS.HostNorm()
    _call_both(env, twin, *OS.observations(4160, seed=1), True, True, 'first')
    _call_both(env, twin, *OS.observations(4160, seed=2, dtype=np.float64), True, True, 'second')
    _call_both(env, twin, *OS.observations(4097, seed=3), True, False, 'third')
    assert twin.n_state == 2 * 4160 + 4097
    env.close()


def test_set_get_round_trip_and_loaded_statistics():
    """obsnorm_load then obsnorm_state round-trips exactly; statistics loaded from a BatchedStateNorm normalise bit-equal to it, for
    float32 and float64 observations; DeviceStateNorm hands them over both ways"""
    from hope_amd import ParkingBatch
    from hope_amd import agent_glue as G
    env = ParkingBatch(130, 32)
    env.enable_obsnorm()
    dev = env.device
    rng = np.random.default_rng(4)
    mean, S, std = rng.normal(0, 5, OS.NC), rng.uniform(0, 1e6, OS.NC), rng.uniform(0, 9, OS.NC)
    env.obsnorm_load(12345678901, mean, S, std)
    n, m2, S2, std2 = env.obsnorm_state()
    assert n == 12345678901 == env.obsnorm_count()
    assert all(np.array_equal(OS.words(a), OS.words(b)) for a, b in ((mean, m2), (S, S2), (std, std2)))
    sb = G.BatchedStateNorm(device=dev)
    for k in range(3):
        lidar, target = (torch.from_numpy(a).to(dev) for a in OS.observations(130, seed=30 + k))
        sb.update({'lidar': lidar, 'target': target})
    dn = G.DeviceStateNorm(env, from_norm=sb)
    assert dn.on_device and dn.n_state == sb.n_state == 390
    for name in ('mean', 'S', 'std'):
        assert all(torch.equal(getattr(dn, name)[k], getattr(sb, name)[k]) for k in sb.modal), name
    back = dn.to_batched()
    assert back.n_state == 390 and all(torch.equal(back.std[k], sb.std[k]) and back.std[k].device == dev for k in sb.modal)
    for dt in (np.float32, np.float64):
        lq, tq = OS.observations(77, seed=40, dtype=dt)
        if dt == np.float64:                                       # values that are no float32
            lq, tq = lq * (1.0 + 2.0 ** -40), tq / 3.0
        obs = {'lidar': torch.from_numpy(lq).to(dev), 'target': torch.from_numpy(tq).to(dev)}
        got, want = dn.normalize(obs), sb.normalize(obs)
        for k in sb.modal:
            assert got[k].dtype == torch.float32 and got[k].shape == want[k].shape
            assert torch.equal(got[k].view(torch.int32), want[k].float().view(torch.int32)), (dt, k)
    assert env.obsnorm_count() == 390                              # normalising folded nothing in
    env.close()


def test_device_norm_inside_the_step_loop_follows_the_torch_path():
    """512 generated lots (mixed_arrays, seed 7, max_obst 32), 24 deferred fused-turnover steps of a HopeRollout whose actions come
    from the torch path (BatchedStateNorm, device planner).  The same raw observations go to the device norm.  After every step:
      statistics   |mean - torch|, |std - torch| <= 1e-11 max(1, max|x|) per column -- torch's unordered float64 sum over at most
                   65 536 rows is bounded by N 2^-53 ~ 7e-12 of max|x|, the fixed rule's share is negligible;
      observation  |out - torch| <= 1e-5 max(1, |value|) -- the float64 quotients differ far below one float32 ulp, so only rounding
                   ties move a float32 value, by one ulp.
    Seen on an MI355X: mean 1.4e-16, std 1.1e-16 of the scale; 0 of 1 600 000 float32 values differ.
    Then PPOTrainer(obs_norm='device', chooser='device', use_planner='device') for two updates: finite losses, and n_state is the
    count the host expects, 512 x (1 + steps)."""
    from hope_amd import ParkingBatch
    from hope_amd import agent_glue as G
    from hope_amd import agents as A
    from hope_amd.rollout import HopeRollout, PPOTrainer
    arrs = OS.loop_arrays()
    env = ParkingBatch(OS.LOOP_LOTS, 32)
    env.set_scene_arrays(np.arange(OS.LOOP_LOTS), *arrs[:5])
    env.enable_obsnorm()
    dev = env.device
    torch.manual_seed(0)
    agent = A.BatchedPPO(device=dev, use_img=False)
    ro = HopeRollout(env, agent, horizon=OS.LOOP_STEPS, seed=1, use_planner='device')          # reset_obs + observe(first observation)
    assert ro.obs_norm is None and isinstance(agent.state_norm, G.BatchedStateNorm) and ro.defer_rs
    amax = torch.ones(OS.NC, dtype=torch.float64, device=dev)
    worst = {'mean': 0.0, 'std': 0.0, 'obs': 0.0}
    moved = 0
    for t in range(OS.LOOP_STEPS + 1):
        if t:
            ro.collect_step()                                      # act (torch norm) -> step -> observe
        raw = torch.cat([env.lidar, env.target], dim=1).double()
        amax = torch.maximum(amax, raw.abs().max(dim=0).values)
        nl, nt = env.obsnorm()                                     # fold, then normalise with the new statistics
        want = agent._norm_obs(ro._raw_obs())
        n, mean, _, std = env.obsnorm_state()
        sn = agent.state_norm
        assert n == sn.n_state == OS.LOOP_LOTS * (t + 1)
        for name, got, ref in (('mean', mean, sn.mean), ('std', std, sn.std)):
            ref = torch.cat([ref['lidar'], ref['target']])
            err = float(((torch.from_numpy(got).to(dev) - ref).abs() / amax).max())
            worst[name] = max(worst[name], err)
            assert err <= 1e-11, (t, name, err)
        got, ref = torch.cat([nl, nt], dim=1), torch.cat([want['lidar'], want['target']], dim=1)
        assert ref.dtype == torch.float32
        err = float(((got.double() - ref.double()).abs() / ref.double().abs().clamp(min=1.0)).max())
        worst['obs'] = max(worst['obs'], err)
        moved += int((got != ref).sum())
        assert err <= 1e-5, (t, err)
    print('worst', worst, 'float32 values that differ:', moved, 'of', (OS.LOOP_STEPS + 1) * OS.LOOP_LOTS * OS.NC)
    env.close()
    env = ParkingBatch(OS.LOOP_LOTS, 32)
    env.set_scene_arrays(np.arange(OS.LOOP_LOTS), *arrs[:5])
    torch.manual_seed(0)
    ag = A.BatchedPPO(device=dev, use_img=False, mini_batch=OS.LOOP_LOTS * 4, mini_epoch=1)
    tr = PPOTrainer(env, ag, horizon=4, seed=2, use_planner='device', chooser='device', obs_norm='device')
    assert isinstance(ag.state_norm, G.DeviceStateNorm) and ag.state_norm.on_device and tr.obs_norm is ag.state_norm
    losses = [x for x in (tr.step() for _ in range(8)) if x is not None]
    assert tr.updates == 2 and len(losses) == 2 and all(math.isfinite(float(v)) for l_ in losses for v in l_), losses
    assert ag.state_norm.n_state == OS.LOOP_LOTS * (1 + 8)
    assert all(torch.isfinite(v).all() for v in ag.state_norm.std.values())
    env.close()


def test_misuse_fails_loudly():
    """HOPE_ESTATE before enable; HOPE_EINVAL for rows of 0 and N + 1, no flag, an unknown flag, NORMALIZE without outputs, NULL
    or misaligned inputs -- every one refused before anything is launched; disable and enable again starts from nothing"""
    from hope_amd import ParkingBatch
    from hope_amd import _lib as L
    n = 70
    env = ParkingBatch(n, 32)
    dev, lib = env.device, env.lib
    lidar = torch.zeros((n + 1, 120), device=dev)
    target = torch.zeros((n + 1, 5), device=dev)
    ol, ot = torch.zeros((n, 120), device=dev), torch.zeros((n, 5), device=dev)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    U, N = L.OBSNORM_UPDATE, L.OBSNORM_NORMALIZE

    def raw(lidar=lidar, target=target, rows=n, in_f64=0, flags=U | N, ol=ol, ot=ot):
        return lib.hope_env_obsnorm(env.h, P(lidar), P(target), rows, in_f64, flags, P(ol), P(ot), env._stream())
    assert raw() == -5 and b'normalisation is off' in lib.hope_last_error()             # HOPE_ESTATE
    z = np.zeros(OS.NC)
    assert lib.hope_env_obsnorm_set(env.h, 0, z.ctypes.data, z.ctypes.data, z.ctypes.data) == -5
    assert lib.hope_env_obsnorm_get(env.h, None, None, None, None) == -5
    with pytest.raises(L.HopeError, match='code -5'):
        env.obsnorm()
    env.enable_obsnorm()
    assert raw() == 0 and raw(flags=U, ol=None, ot=None) == 0 and raw(rows=1) == 0
    assert env.obsnorm_count() == 2 * n + 1
    for kw in ({'rows': 0}, {'rows': n + 1}, {'rows': -3}, {'flags': 0}, {'flags': 4}, {'flags': N, 'ol': None}, {'flags': U | N, 'ot': None},
               {'lidar': None}, {'target': None}, {'lidar': lidar.view(-1)[1:], 'in_f64': 1}, {'target': target.view(-1)[1:], 'in_f64': 1}):
        assert raw(**kw) == -1, kw                                                     # HOPE_EINVAL
    assert lib.hope_env_obsnorm_set(env.h, -1, z.ctypes.data, z.ctypes.data, z.ctypes.data) == -1
    assert lib.hope_env_obsnorm_set(env.h, 0, None, z.ctypes.data, z.ctypes.data) == -1
    assert env.obsnorm_count() == 2 * n + 1                                            # the refused calls folded nothing in
    for kw in (dict(lidar=lidar[:n].double()), dict(lidar=lidar[:n, :119]), dict(target=target[:n - 1]), dict(lidar=lidar[:n].cpu()),
               dict(lidar=torch.zeros((120, n), device=dev).t()), dict(lidar=lidar, target=target)):
        args = dict(lidar=lidar[:n], target=target[:n])
        args.update(kw)
        with pytest.raises(L.HopeError):
            env.obsnorm(**args)
    env.disable_obsnorm()
    assert raw() == -5
    env.enable_obsnorm()
    assert env.obsnorm_count() == 0
    env.disable_obsnorm()
    env.disable_obsnorm()                                                              # (idempotent, like the chooser's)
    env.close()
