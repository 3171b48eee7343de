"""k_sac_sample / k_sac_critic / k_sac_seed / k_sac_policy / k_sac_merge (hope_amd/csrc/hope_sac_kernel.h) on the device: word for word
their host twins, ordered by the stream they are enqueued on, misused, in the reference's recorded update and inside SACTrainer."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sac_update_script as S  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_BATCH = 4097                                      # 65 chunk partials: more than the merge wave has lanes, with an odd one
NAMES = {'sample': ('action', 'lp'), 'critic': ('q_target', 'g_q1', 'g_q2', 'losses'), 'seed': ('s1', 's2'),
         'policy': ('g_raw', 'g_log_std', 'g_log_alpha', 'losses')}


@pytest.fixture(scope='module')
def env():
    from hope_amd import ParkingBatch
    e = ParkingBatch(64, 32)
    e.enable_sac_update(MAX_BATCH)
    yield e
    e.close()


def _dev(env, a, offset=0):
    """the array on the device; offset = 1: in a buffer whose base is 4 bytes past the allocation's (only 4-byte aligned)"""
    a = np.asarray(a)
    if not offset or a.dtype.itemsize != 4:                     # (log_alpha, a float64 scalar, keeps its 8 bytes)
        return torch.from_numpy(a.copy()).to(env.device)
    a = np.ascontiguousarray(a)
    buf = torch.zeros(a.size + offset, dtype=torch.from_numpy(a).dtype, device=env.device)
    v = buf[offset:].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 8 == 4 * offset and v.is_contiguous()
    return v


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(S.words(got), S.words(want)), what


def _device_all(env, t):
    """the four calls over the device tensors t (keys as S.inputs) -> {call: outputs}"""
    return {'sample': env.sac_sample(t['raw'], t['log_std'], t['eps']),
            'critic': env.sac_critic(t['q1'], t['q2'], t['qt1'], t['qt2'], t['next_lp'], t['reward'], t['done'], t['log_alpha'], S.GAMMA),
            'seed': env.sac_seed(t['p1'], t['p2']),
            'policy': env.sac_policy(t['raw'], t['log_std'], t['eps'], t['p1'], t['p2'], t['g_action'], t['log_alpha'], S.TARGET_ENTROPY)}


@pytest.mark.parametrize('b', [1, 63, 64, 65, 129, 4097])
def test_kernels_equal_the_host_twins_word_for_word(env, b):
    """every output of the four calls, g_log_alpha as a float64 word, from 8-byte aligned bases (the float2 path) and from bases 4
    bytes past the allocation's (the 4-byte path), inputs and outputs"""
    x = S.inputs(b)
    want = S.host_all(x)
    for offset in (0, 1):
        t = {k: _dev(env, v, offset) for k, v in x.items()}
        got = _device_all(env, t)
        for call, outs in got.items():
            assert all(o is p for o, p in zip(outs, env._sac_out[(call, b)]))                  # persistent per batch size
            for o, w, what in zip(outs, want[call], NAMES[call]):
                _same(o, w, (b, offset, call, what))
    # outputs that are only 4-byte aligned: the C calls with their own buffers
    P = lambda q: C.c_void_p(q.data_ptr())  # noqa: E731
    t = {k: _dev(env, v) for k, v in x.items()}
    f32 = lambda *shape: _dev(env, np.zeros(shape, np.float32), 1)  # noqa: E731
    lib, h, st = env.lib, env.h, env._stream()
    out = {'sample': [f32(b, 2), f32(b)], 'critic': [f32(b), f32(b), f32(b), f32(2)], 'seed': [f32(b), f32(b)],
           'policy': [f32(b, 2), f32(2), torch.zeros((), dtype=torch.float64, device=env.device), f32(2)]}
    assert lib.hope_env_sac_sample(h, P(t['raw']), P(t['log_std']), P(t['eps']), b, *map(P, out['sample']), st) == 0
    assert lib.hope_env_sac_critic(h, *(P(t[k]) for k in ('q1', 'q2', 'qt1', 'qt2', 'next_lp', 'reward', 'done', 'log_alpha')), S.GAMMA, b,
                                   *map(P, out['critic']), st) == 0
    assert lib.hope_env_sac_seed(h, P(t['p1']), P(t['p2']), b, *map(P, out['seed']), st) == 0
    assert lib.hope_env_sac_policy(h, *(P(t[k]) for k in ('raw', 'log_std', 'eps', 'p1', 'p2', 'g_action', 'log_alpha')), S.TARGET_ENTROPY, b,
                                   *map(P, out['policy']), st) == 0
    for call, outs in out.items():
        for o, w, what in zip(outs, want[call], NAMES[call]):
            _same(o, w, (b, 'offset outputs', call, what))


def test_the_calls_are_ordered_by_their_stream(env):
    """inputs produced by torch on a side stream, the four calls enqueued there, the results copied back there: nothing synchronises
    the host in between (the copies to the host wait for that stream only)"""
    b = 4097
    x = S.inputs(b, seed=9)
    side = torch.cuda.Stream(device=env.device)
    hx = {k: torch.from_numpy(np.asarray(v).copy()).pin_memory() for k, v in x.items()}
    torch.cuda.synchronize(env.device)
    with torch.cuda.stream(side):
        dx = {k: v.to(env.device, non_blocking=True) for k, v in hx.items()}
        for _ in range(40):                                        # some work in front of the values the calls read
            dx = {k: (v * 2.0) * 0.5 for k, v in dx.items()}
        got = {call: [o.cpu() for o in outs] for call, outs in _device_all(env, dx).items()}
    want = S.host_all(x)
    for call, outs in got.items():
        for o, w, what in zip(outs, want[call], NAMES[call]):
            _same(o, w, (call, what))
    torch.cuda.synchronize(env.device)


def test_misuse_fails_loudly():
    """HOPE_ESTATE before enable; HOPE_EINVAL, each with its text, for a batch of 0 and max_batch + 1, a NULL pointer, a misaligned
    pointer, a gamma or target_entropy that is not finite -- each refused before anything is launched; the handle gives the twins'
    words afterwards; enable, disable, enable again; a re-enable with a larger max_batch"""
    from hope_amd import ParkingBatch
    from hope_amd import _lib as L
    mb = 100
    e = ParkingBatch(16, 32)
    dev, lib = e.device, e.lib
    x = S.inputs(mb + 1)
    t = {k: torch.from_numpy(v).to(dev) for k, v in x.items()}
    o = {'action': torch.zeros(mb + 1, 2, device=dev), 'lp': torch.zeros(mb + 1, device=dev), 'q_target': torch.zeros(mb + 1, device=dev),
         'g_q1': torch.zeros(mb + 1, device=dev), 'g_q2': torch.zeros(mb + 1, device=dev), 'losses': torch.zeros(2, device=dev),
         's1': torch.zeros(mb + 1, device=dev), 's2': torch.zeros(mb + 1, device=dev), 'g_raw': torch.zeros(mb + 1, 2, device=dev),
         'g_log_std': torch.zeros(2, device=dev), 'g_log_alpha': torch.zeros((), dtype=torch.float64, device=dev)}
    err = lambda: lib.hope_last_error().decode()  # noqa: E731
    sig = {'sample': (('raw', 'log_std', 'eps'), None, ('action', 'lp')),
           'critic': (('q1', 'q2', 'qt1', 'qt2', 'next_lp', 'reward', 'done', 'log_alpha'), S.GAMMA, ('q_target', 'g_q1', 'g_q2', 'losses')),
           'seed': (('p1', 'p2'), None, ('s1', 's2')),
           'policy': (('raw', 'log_std', 'eps', 'p1', 'p2', 'g_action', 'log_alpha'), S.TARGET_ENTROPY, ('g_raw', 'g_log_std', 'g_log_alpha', 'losses'))}

    def call(name, batch=mb, scalar=None, **ptr):
        """hope_env_sac_<name> with pointer arguments replaced by ptr[argument] (None: NULL, an int: that address)"""
        ins, default, outs = sig[name]
        P = lambda k, q: C.c_void_p(q.data_ptr()) if k not in ptr else (None if ptr[k] is None else C.c_void_p(ptr[k]))  # noqa: E731
        a = [P(k, t[k]) for k in ins] + ([] if default is None else [default if scalar is None else scalar]) + [batch] + [P(k, o[k]) for k in outs]
        return getattr(lib, 'hope_env_sac_' + name)(e.h, *a, e._stream())
    for name in sig:
        assert call(name) == -5 and f'hope_env_sac_{name}: the SAC update is off (hope_env_sac_enable first)' in err()           # HOPE_ESTATE
    for bad in (0, -1, L.SAC_MAX_BATCH + 1):
        assert lib.hope_env_sac_enable(e.h, bad) == -1 and 'hope_env_sac_enable: max_batch must be 1 .. 1048576' in err()
    e.enable_sac_update(mb)
    for name, (ins, default, outs) in sig.items():
        assert call(name) == 0 and call(name, batch=1) == 0
        for kw, text in [({'batch': 0}, 'batch must be 1 .. max_batch (100)'), ({'batch': mb + 1}, 'batch must be 1 .. max_batch (100)')] + \
                [({k: None}, 'null ') for k in ins + outs] + [({k: (t[k] if k in t else o[k]).data_ptr() + 2}, 'misaligned buffer') for k in (ins[0], outs[0])]:
            assert call(name, **kw) == -1 and f'hope_env_sac_{name}: ' in err() and text in err(), (name, kw, err())                 # HOPE_EINVAL
        if default is not None:
            for v in (float('nan'), float('inf'), -float('inf')):
                assert call(name, scalar=v) == -1 and 'must be finite' in err(), (name, v, err())
    for name, k in (('critic', 'log_alpha'), ('policy', 'log_alpha'), ('policy', 'g_log_alpha')):                                  # float64: 8 bytes
        q = t[k] if k in t else o[k]
        assert call(name, **{k: q.data_ptr() + 4}) == -1 and 'misaligned buffer (log_alpha' in err(), (name, k, err())

    def words_after(batch):
        """the handle is as usable as before: real calls give the twins' words"""
        xb = S.inputs(batch)
        got = _device_all(e, {k: torch.from_numpy(v).to(dev) for k, v in xb.items()})
        want = S.host_all(xb)
        for c, outs in got.items():
            for g, w, what in zip(outs, want[c], NAMES[c]):
                _same(g, w, ('after', batch, c, what))
    words_after(mb)
    with pytest.raises(L.HopeError, match=r'hope_env_sac_sample: eps must be float32 \[100, 2\]'):
        e.sac_sample(t['raw'][:mb], t['log_std'], t['eps'][:mb - 1])
    with pytest.raises(L.HopeError, match=r'hope_env_sac_critic: log_alpha must be float64 \[\]'):
        e.sac_critic(*(t[k][:mb] for k in ('q1', 'q2', 'qt1', 'qt2', 'next_lp', 'reward', 'done')), t['log_alpha'].float(), S.GAMMA)
    with pytest.raises(L.HopeError, match='hope_env_sac_seed failed'):
        e.sac_seed(t['p1'], t['p2'])                                                   # mb + 1 items: past max_batch
    e.disable_sac_update()
    assert all(call(name) == -5 for name in sig)
    e.enable_sac_update(mb)
    e.enable_sac_update(mb // 2)                                                       # (equal or smaller: nothing changes)
    assert call('policy') == 0 and call('policy', batch=mb + 1) == -1
    words_after(mb)
    e.enable_sac_update(mb + 1)                                                        # larger: the partials are reallocated
    assert call('critic', batch=mb + 1) == 0 and call('critic', batch=mb + 2) == -1
    words_after(mb + 1)
    e.disable_sac_update()
    e.disable_sac_update()
    e.close()


def test_reference_recording_on_the_gpu(env):
    """the reference's recorded SAC update (tests/golden/sac_update.npz; test_agents.check_sac_update's scenario) on `cuda` with the
    update block over the library's kernels, at test_gpu_agents.py's tolerance for it"""
    import test_agents as TA
    from hope_amd import agent_glue as G
    from hope_amd import agents as A
    tol, dev = 3e-3, 'cuda'
    g = TA._load('sac_update.npz')
    blk = G.make_sac_update('device', env)
    assert blk.on_device
    ag = A.BatchedSAC(device=dev, use_img=True, lr=2e-4, batch_size=16, state_norm=False, update_block=blk)
    TA.det_fill(ag.actor, 0.1)
    TA.det_fill(ag.critic1, 0.3)
    TA.det_fill(ag.critic2, 0.4)
    ag.critic_target1.load_state_dict(ag.critic1.state_dict())
    ag.critic_target2.load_state_dict(ag.critic2.state_dict())
    with torch.no_grad():
        ag.log_std.copy_(torch.tensor([[-0.5, -0.1]], device=dev))
    f = lambda k: torch.from_numpy(g[k]).to(dev)  # noqa: E731
    batch = {'obs': TA._obs(g, 'x_', dev), 'next_obs': TA._obs(g, 'nx_', dev), 'action': f('action'), 'reward': f('reward'), 'done': f('done')}
    eps = f('eps')
    for u in range(3):
        a, b = ag.update(batch, noise=(eps[2 * u], eps[2 * u + 1]))
        assert abs(a - g['losses'][u, 0]) < tol * max(1, abs(g['losses'][u, 0])), (u, a, g['losses'][u])
        assert abs(b - g['losses'][u, 1]) < tol * max(1, abs(g['losses'][u, 1])), (u, b, g['losses'][u])
    for name, net in (('probe_actor', ag.actor), ('probe_q1', ag.critic1), ('probe_q2', ag.critic2), ('probe_t1', ag.critic_target1),
                      ('probe_t2', ag.critic_target2)):
        got, exp = TA.probe(net.cpu()).numpy(), g[name]
        assert (np.abs(got - exp) / np.maximum(np.abs(exp[:, 1:2]), 1.0)).max() < tol, name
    assert abs(float(ag.log_alpha.detach()) - float(g['log_alpha'])) < 1e-5
    assert np.allclose(ag.log_std.detach().cpu().numpy(), g['log_std'], atol=tol)


def test_trainer_with_the_device_update():
    """SACTrainer(ring='device', sac_update='device'): 64 generated lots, horizon 4, a batch of 64, three updates -- finite losses; every
    call of every update, intercepted with the very tensors it was given, equals the host twin on the same inputs, word for word"""
    from hope_amd import ParkingBatch
    from hope_amd import agent_glue as G
    from hope_amd import agents as A
    from hope_amd.rollout import SACTrainer
    from hope_amd.scene_gen import mixed_arrays
    n, horizon, every, b = 64, 4, 2, 64
    arrs = mixed_arrays(n, levels=('Normal', 'Complex', 'Extrem'), seed=11, max_obst=32)
    e = ParkingBatch(n, 32)
    e.set_scene_arrays(np.arange(n), *arrs[:5])
    torch.manual_seed(0)
    ag = A.BatchedSAC(device=e.device, use_img=False, batch_size=b)
    tr = SACTrainer(e, ag, horizon=horizon, update_every=every, seed=3, use_planner='device', ring='device', sac_update='device')
    assert isinstance(ag.update_block, G.DeviceSacUpdate) and ag.update_block.on_device and tr.sac_update is ag.update_block
    seen = []
    for name in ('sac_sample', 'sac_critic', 'sac_seed', 'sac_policy'):
        def spy(*args, _inner=getattr(e, name), _name=name):
            out = _inner(*args)
            seen.append((_name, [a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a for a in args], [o.cpu().numpy() for o in out]))
            return out
        setattr(e, name, spy)
    out = [tr.step() for _ in range(horizon + 2 * every)]
    losses = [o for o in out if o is not None]
    assert tr.updates == 3 and len(losses) == 3 and all(math.isfinite(float(v)) for l_ in losses for v in l_), losses
    assert [s[0] for s in seen] == ['sac_sample', 'sac_critic', 'sac_sample', 'sac_seed', 'sac_policy'] * 3
    for u in range(3):
        (_, a0, o0), (_, a1, o1), (_, a2, o2), (_, a3, o3), (_, a4, o4) = seen[5 * u:5 * u + 5]
        for (raw, log_std, eps), o in ((a0, o0), (a2, o2)):
            assert raw.shape == (b, 2) and float(np.abs(raw).max()) > 0 and float(np.abs(eps).max()) > 0
            for g, w, what in zip(o, S.host_sample({'raw': raw, 'log_std': log_std, 'eps': eps}), NAMES['sample']):
                _same(g, w, (u, 'sample', what))
        x = dict(zip(('q1', 'q2', 'qt1', 'qt2', 'next_lp', 'reward', 'done', 'log_alpha'), a1[:8]))
        assert np.array_equal(S.words(x['next_lp']), S.words(o0[1]))                       # the critic call read the first sample's lp
        for g, w, what in zip(o1, S.host_critic(x, gamma=a1[8]), NAMES['critic']):
            _same(g, w, (u, 'critic', what))
        for g, w, what in zip(o3, S.host_seed({'p1': a3[0], 'p2': a3[1]}), NAMES['seed']):
            _same(g, w, (u, 'seed', what))
        x = dict(zip(('raw', 'log_std', 'eps', 'p1', 'p2', 'g_action', 'log_alpha'), a4[:7]))
        assert float(np.abs(x['g_action']).max()) > 0 and np.array_equal(x['raw'], a2[0]) and np.array_equal(x['eps'], a2[2])
        for g, w, what in zip(o4, S.host_policy(x, target_entropy=a4[7]), NAMES['policy']):
            _same(g, w, (u, 'policy', what))
        assert losses[u] == (float(o4[3][0]), float(o1[3][0]))
    e.close()
