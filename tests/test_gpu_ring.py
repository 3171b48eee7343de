"""k_ring_before / k_ring_after / k_ring_tally / k_ring_sample (hope_amd/csrc/hope_ring_kernel.h) on the device: word for word their
host twins, ordered by the stream they are enqueued on, misused, and inside PPOTrainer and SACTrainer."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ring_script as RS  # noqa: E402

pytestmark = pytest.mark.gpu

N = 193


@pytest.fixture(scope='module')
def env():
    from hope_amd import ParkingBatch
    e = ParkingBatch(N, 32)
    e.enable_ring()
    yield e
    e.close()


def _dev(env, a, offset=0):
    """the array on the device; offset = 1: in a buffer whose base is one element past the allocation's (float32: only 4-byte aligned)"""
    a = np.ascontiguousarray(a)
    if not offset:
        return torch.from_numpy(a).to(env.device)
    buf = torch.zeros(a.size + 1, dtype=torch.from_numpy(a).dtype, device=env.device)
    v = buf[1:].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == a.itemsize and v.is_contiguous()
    return v


def _dev_ring(env, ring, offset):
    from hope_amd import _lib as L
    t = {k: _dev(env, v, offset) for k, v in ring.items()}
    n, horizon = ring['reward'].shape
    return t, L.ring_desc('test', env.device, n, horizon, **t)


def _same(got, want, what):
    assert tuple(got.shape) == tuple(want.shape) and np.array_equal(RS.words(got), RS.words(want)), what


@pytest.mark.parametrize('n', RS.NS)
def test_push_and_tally_equal_the_host_twins_word_for_word(env, n):
    """T + 3 pushes per T, float32 and float64 rewards in turn, the tally on two steps of three: the ring tensors, counts and
    reward_sum (as uint64 words) after every T's run, from 16-byte aligned bases (a lane moves 16 / 8 bytes) and from bases one
    element further (4 bytes)"""
    for t in RS.TS:
        for offset in (0, 1):
            host = RS.np_ring(n, t, fill=7.0)
            dev, d = _dev_ring(env, host, offset)
            assert dev['lidar'].data_ptr() % 16 == 4 * offset
            counts, rsum = np.array([3, 1], np.int64), np.array([0.5])
            dcounts, dsum = _dev(env, counts, offset), _dev(env, rsum, offset)
            for step in range(t + 3):
                x = RS.step_inputs(n, step, f64=bool(step % 2))
                tally = step % 3 != 2
                RS.host_before(host, step % t, x)
                RS.host_after(host, step % t, x, *((counts, rsum) if tally else ()))
                dx = {k: _dev(env, v, offset) for k, v in x.items()}
                env.ring_before(d, step % t, dx['lidar'], dx['target'], dx['action_mask'], dx['action'], dx['log_prob'])
                env.ring_after(d, step % t, dx['reward'], dx['done'], *((dx['status'], dcounts, dsum) if tally else ()))
            for k in host:
                _same(dev[k], host[k], (n, t, offset, k))
            _same(dcounts, counts, (n, t, offset, 'counts'))
            _same(dsum, rsum, (n, t, offset, 'reward_sum'))


@pytest.mark.parametrize('n', RS.NS)
def test_sample_equals_the_host_twin_word_for_word(env, n):
    """supplied (s, j) -- size < T, size == T with the head at 0 and in the middle, the newest column, the one before it, T = 1, a
    repeated pair, rows out of range -- and drawn ones, batches of 1, 32, 65, 257, aligned and offset bases: every output and idx"""
    from hope_amd import _lib as L
    from hope_amd.rollout import ring_draws
    last = RS.last_obs(n)
    for t, pushes in RS.SAMPLE_STATES:
        host, head, size = RS.filled_ring(n, t, pushes, f64=bool(pushes % 2))
        for offset in (0, 1):
            _, d = _dev_ring(env, host, offset)
            dl = [_dev(env, last[k], offset) for k in RS.KEYS]
            for batch in RS.BATCHES:
                s, j = RS.case_index(n, size, batch)
                if batch > 32:                                     # refused rows among good ones
                    s[5], j[7], s[batch - 1] = n, -1, -1
                for mode in ('supplied', 'drawn'):
                    out = {k: _dev(env, v, offset) for k, v in RS.batch_arrays(batch).items()}
                    od = L.ring_batch_desc('test', env.device, batch, **out)
                    if mode == 'supplied':
                        want = RS.host_sample(host, head, size, batch, last, s, j)
                        env.ring_sample(d, head, size, batch, od, *dl, s=_dev(env, s, offset), j=_dev(env, j, offset))
                    else:
                        want = RS.host_sample(host, head, size, batch, last, seed=n + t, counter=batch)
                        env.ring_sample(d, head, size, batch, od, *dl, seed=n + t, counter=batch)
                        ds, dj = ring_draws(n + t, batch, batch, n, size)
                        assert np.array_equal(want['idx'], RS.expected_idx(head, size, t, ds, dj))
                    for k in want:
                        _same(out[k], want[k], (n, t, pushes, offset, batch, mode, k))
                if batch > 32:
                    assert (want['idx'] >= 0).any()                # (drawn: no refused rows)


def test_the_calls_are_ordered_by_their_stream(env):
    """inputs produced by torch on a side stream, push, tally and batch enqueued there, the results copied back there: nothing
    synchronises the host in between"""
    from hope_amd import _lib as L
    n, t, batch = N, 5, 65
    host = RS.np_ring(n, t)
    last = RS.last_obs(n)
    xs = [RS.step_inputs(n, step, f64=bool(step % 2)) for step in range(3)]
    counts, rsum = np.zeros(2, np.int64), np.zeros(1)
    for step, x in enumerate(xs):
        RS.host_before(host, step, x)
        RS.host_after(host, step, x, counts, rsum)
    want = RS.host_sample(host, 3, 3, batch, last, seed=5, counter=9)
    side = torch.cuda.Stream(device=env.device)
    pinned = [{k: torch.from_numpy(v).pin_memory() for k, v in x.items()} for x in xs]
    pl = [torch.from_numpy(last[k]).pin_memory() for k in RS.KEYS]
    dev, d = _dev_ring(env, RS.np_ring(n, t), 0)
    out = {k: _dev(env, v) for k, v in RS.batch_arrays(batch).items()}
    od = L.ring_batch_desc('test', env.device, batch, **out)
    dcounts, dsum = _dev(env, np.zeros(2, np.int64)), _dev(env, np.zeros(1))
    torch.cuda.synchronize(env.device)
    with torch.cuda.stream(side):
        for step, p in enumerate(pinned):
            dx = {k: v.to(env.device, non_blocking=True) for k, v in p.items()}
            for _ in range(20):                                    # some work in front of the values the calls read
                dx = {k: (v * 2.0) * 0.5 if v.is_floating_point() else v + 0 for k, v in dx.items()}
            env.ring_before(d, step, dx['lidar'], dx['target'], dx['action_mask'], dx['action'], dx['log_prob'])
            env.ring_after(d, step, dx['reward'], dx['done'], dx['status'], dcounts, dsum)
        dl = [(v.to(env.device, non_blocking=True) * 2.0) * 0.5 for v in pl]
        env.ring_sample(d, 3, 3, batch, od, *dl, seed=5, counter=9)
        got = {k: v.cpu() for k, v in out.items()}
        got_ring = {k: v.cpu() for k, v in dev.items()}
        got_tally = (dcounts.cpu(), dsum.cpu())
    for k in want:
        _same(got[k], want[k], k)
    for k in host:
        _same(got_ring[k], host[k], k)
    _same(got_tally[0], counts, 'counts'); _same(got_tally[1], rsum, 'reward_sum')
    torch.cuda.synchronize(env.device)


def test_misuse_fails_loudly():
    """HOPE_ESTATE before enable; HOPE_EINVAL for every NULL, misaligned pointer and number out of range -- each with its text, each
    refused before anything is launched (the buffers keep their fill); the handle works afterwards; enable, disable, enable again"""
    from hope_amd import ParkingBatch
    from hope_amd import _lib as L
    n, t, batch = 70, 4, 8
    e = ParkingBatch(n, 32)
    dev, lib = e.device, e.lib
    host = RS.np_ring(n, t, fill=7.0)
    ring, d = _dev_ring(e, host, 0)
    x = {k: _dev(e, v) for k, v in RS.step_inputs(n, 0).items()}
    x64 = _dev(e, RS.step_inputs(n, 0, f64=True)['reward'])
    last = [_dev(e, v) for v in RS.last_obs(n).values()]
    out = {k: _dev(e, v) for k, v in RS.batch_arrays(batch).items()}
    od = L.ring_batch_desc('test', dev, batch, **out)
    counts, rsum = torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
    s = torch.zeros(batch, dtype=torch.int32, device=dev)
    P = lambda q: None if q is None else C.c_void_p(q if isinstance(q, int) else q.data_ptr())  # noqa: E731
    err = lambda: lib.hope_last_error().decode()  # noqa: E731

    def before(ring=d, t=0, **kw):
        a = dict(lidar=x['lidar'], target=x['target'], mask=x['action_mask'], action=x['action'], log_prob=x['log_prob'])
        a.update(kw)
        return lib.hope_env_ring_before(e.h, ring, t, *(P(a[k]) for k in ('lidar', 'target', 'mask', 'action', 'log_prob')), e._stream())

    def after(ring=d, t=0, f64=0, **kw):
        a = dict(reward=x['reward'], done=x['done'], status=x['status'], counts=counts, reward_sum=rsum)
        a.update(kw)
        return lib.hope_env_ring_after(e.h, ring, t, P(a['reward']), f64, *(P(a[k]) for k in ('done', 'status', 'counts', 'reward_sum')), e._stream())

    def sample(ring=d, head=1, size=1, batch=batch, out=od, **kw):
        a = dict(s=None, j=None, last_lidar=last[0], last_target=last[1], last_mask=last[2])
        a.update(kw)
        return lib.hope_env_ring_sample(e.h, ring, head, size, batch, P(a['s']), P(a['j']), 0, 0, *(P(a[k]) for k in ('last_lidar', 'last_target', 'last_mask')),
                                        out, e._stream())

    def changed(base, **kw):
        r = type(base)()
        C.memmove(C.byref(r), C.byref(base), C.sizeof(base))
        for k, v in kw.items():
            setattr(r, k, v)
        return r
    off = 'the transition ring is off (hope_env_ring_enable first)'
    for call, name in ((before, 'hope_env_ring_before'), (after, 'hope_env_ring_after'), (sample, 'hope_env_ring_sample')):
        assert call() == -5 and f'{name}: {off}' in err()                                                            # HOPE_ESTATE
    with pytest.raises(L.HopeError, match='code -5'):
        e.ring_before(d, 0, x['lidar'], x['target'], x['action_mask'], x['action'], x['log_prob'])
    e.enable_ring()
    odd = x['lidar'].data_ptr() + 2
    ring_cases = (({'ring': None}, 'null ring'), ({'ring': changed(d, reward=None)}, 'null tensor in the ring'),
                  ({'ring': changed(d, lidar=ring['lidar'].data_ptr() + 2)}, 'misaligned buffer'), ({'ring': changed(d, n=0)}, "the ring's n must be 1 .. the handle"),
                  ({'ring': changed(d, n=n + 1)}, "the ring's n must be"), ({'ring': changed(d, T=0)}, "the ring's T must be 1 .. 4096"),
                  ({'ring': changed(d, T=4097)}, "the ring's T must be 1 .. 4096"))
    for kw, text in ring_cases + (({'t': -1}, 't must be 0 .. T - 1'), ({'t': t}, 't must be 0 .. T - 1'), ({'lidar': None}, 'null lidar / target'),
                                  ({'log_prob': None}, 'null lidar / target'), ({'mask': odd}, 'misaligned buffer')):
        assert before(**kw) == -1 and 'hope_env_ring_before: ' in err() and text in err(), (kw, err())                # HOPE_EINVAL
    for kw, text in ring_cases + (({'t': -1}, 't must be 0 .. T - 1'), ({'t': t}, 't must be 0 .. T - 1'), ({'reward': None}, 'null reward / done'),
                                  ({'done': None}, 'null reward / done'), ({'status': None}, 'go together'), ({'counts': None}, 'go together'),
                                  ({'reward_sum': None}, 'go together'), ({'reward': odd}, 'misaligned buffer'),
                                  ({'reward': x64.data_ptr() + 4, 'f64': 1}, 'misaligned buffer'), ({'counts': counts.data_ptr() + 4}, 'misaligned buffer'),
                                  ({'reward_sum': rsum.data_ptr() + 4}, 'misaligned buffer'), ({'status': odd}, 'misaligned buffer')):
        assert after(**kw) == -1 and 'hope_env_ring_after: ' in err() and text in err(), (kw, err())
    for kw, text in ring_cases + (({'head': -1}, 'head must be 0 .. T - 1'), ({'head': t}, 'head must be 0 .. T - 1'), ({'size': 0}, 'size must be 1 .. T'),
                                  ({'size': t + 1}, 'size must be 1 .. T'), ({'batch': 0}, 'batch must be 1 .. 1048576'), ({'batch': 2 ** 20 + 1}, 'batch must be'),
                                  ({'s': s}, 's and j go together'), ({'j': s}, 's and j go together'), ({'last_target': None}, 'null last_lidar'),
                                  ({'out': None}, 'null out'), ({'out': changed(od, idx=None)}, 'null tensor in out'),
                                  ({'out': changed(od, action=out['action'].data_ptr() + 2)}, 'misaligned buffer'), ({'s': s.data_ptr() + 2, 'j': s}, 'misaligned buffer')):
        assert sample(**kw) == -1 and 'hope_env_ring_sample: ' in err() and text in err(), (kw, err())
    torch.cuda.synchronize(dev)
    for k in host:                                                 # nothing was launched: every buffer keeps its fill
        _same(ring[k], host[k], k)
    assert (out['reward'] == 7.0).all() and (out['idx'] == 7).all() and int(counts.sum()) == 0 and float(rsum) == 0.0
    for bad in (dict(lidar=x['lidar'].double()), dict(target=x['target'][:, :4]), dict(mask=x['action_mask'].cpu()), dict(action=x['action'].t())):
        a = dict(lidar=x['lidar'], target=x['target'], mask=x['action_mask'], action=x['action'], log_prob=x['log_prob'])
        a.update(bad)
        with pytest.raises(L.HopeError):
            e.ring_before(d, 0, **a)
    with pytest.raises(L.HopeError):
        e.ring_before(object(), 0, x['lidar'], x['target'], x['action_mask'], x['action'], x['log_prob'])
    with pytest.raises(L.HopeError):
        e.ring_after(d, 0, x['reward'], x['done'].float())
    with pytest.raises(L.HopeError):
        e.ring_sample(d, 1, 1, batch, od, *last, s=s.long(), j=s)
    # the handle is as usable as before: real calls give the twins' words
    xh = RS.step_inputs(n, 0)
    hc, hs = np.zeros(2, np.int64), np.zeros(1)
    RS.host_before(host, 0, xh); RS.host_after(host, 0, xh, hc, hs)
    want = RS.host_sample(host, 1, 1, batch, RS.last_obs(n), seed=3, counter=4)
    for _ in range(2):
        counts.zero_(); rsum.zero_()
        e.ring_before(d, 0, x['lidar'], x['target'], x['action_mask'], x['action'], x['log_prob'])
        e.ring_after(d, 0, x['reward'], x['done'], x['status'], counts, rsum)
        e.ring_sample(d, 1, 1, batch, od, *last, seed=3, counter=4)
        for k in host:
            _same(ring[k], host[k], k)
        for k in want:
            _same(out[k], want[k], k)
        _same(counts, hc, 'counts'); _same(rsum, hs, 'reward_sum')
        e.disable_ring()
        assert before() == -5 and after() == -5 and sample() == -5
        e.enable_ring()
        e.enable_ring()                                            # (idempotent)
    e.disable_ring()
    e.disable_ring()
    e.close()


def _lots(n, seed=11):
    from hope_amd import ParkingBatch
    from hope_amd.scene_gen import mixed_arrays
    arrs = mixed_arrays(n, levels=('Normal', 'Complex', 'Extrem'), seed=seed, max_obst=32)
    e = ParkingBatch(n, 32)
    e.set_scene_arrays(np.arange(n), *arrs[:5])
    return e


def test_ppo_trainer_with_every_device_option():
    """PPOTrainer(ring='device', chooser='device', obs_norm='device', use_planner='device', gae='device') against the same trainer
    with ring=None on 256 generated lots: the ring tensors, the losses of two updates at horizon 4 and the counts of stats() are equal"""
    from hope_amd import agents as A
    from hope_amd.rollout import DeviceTransitionRing, PPOTrainer
    n, runs = 256, []
    for ring in (None, 'device'):
        e = _lots(n)
        torch.manual_seed(0)
        ag = A.BatchedPPO(device=e.device, use_img=False, mini_batch=n * 4, mini_epoch=1)
        tr = PPOTrainer(e, ag, horizon=4, seed=2, use_planner='device', chooser='device', obs_norm='device', gae='device', ring=ring)
        losses = [x for x in (tr.step() for _ in range(8)) if x is not None]
        assert tr.updates == 2 and len(losses) == 2 and all(math.isfinite(float(v)) for l_ in losses for v in l_), losses
        tensors = [tr.ring.obs[k] for k in RS.KEYS] + [tr.ring.action, tr.ring.log_prob, tr.ring.reward, tr.ring.done]
        runs.append(([[float(v) for v in l_] for l_ in losses], [q.cpu().numpy().copy() for q in tensors], tr.stats(),
                     isinstance(tr.ring, DeviceTransitionRing) and tr.ring.on_device))
        e.close()
    (l0, t0, s0, d0), (l1, t1, s1, d1) = runs
    assert d1 and not d0
    assert np.array_equal(np.array(l0).view(np.uint64), np.array(l1).view(np.uint64)), (l0, l1)
    for a, b in zip(t0, t1):
        _same(b, a, 'ring tensors')
    assert s0['steps'] == s1['steps'] == 8 and s0['episodes'] == s1['episodes'] and s0['success_rate'] == s1['success_rate']
    assert math.isfinite(s1['mean_reward']) and s1['episodes'] > 0


def test_sac_trainer_batches_equal_the_twins():
    """SACTrainer(ring='device') for horizon + 2 update_every steps: every update's batch is what the host twin draws from the ring's
    contents at that moment with the ring's seed and counter"""
    from hope_amd import agents as A
    from hope_amd.rollout import SACTrainer
    n, horizon, every, batch = 256, 4, 2, 32
    e = _lots(n, seed=12)
    torch.manual_seed(0)
    ag = A.BatchedSAC(device=e.device, use_img=False, batch_size=batch)
    tr = SACTrainer(e, ag, horizon=horizon, update_every=every, seed=3, use_planner='device', ring='device')
    ring, inner, seen = tr.ring, ag.update, []

    def update(b):
        host = {k: ring.obs[k].cpu().numpy() for k in RS.KEYS}
        host.update(action=ring.action.cpu().numpy(), log_prob=ring.log_prob.cpu().numpy(), reward=ring.reward.cpu().numpy(), done=ring.done.cpu().numpy())
        last = {k: v.float().cpu().numpy() for k, v in tr.last_obs().items() if k in RS.KEYS}
        want = RS.host_sample(host, ring.head, ring.size, batch, last, seed=ring.seed, counter=ring.counter - 1)
        got = {'obs_lidar': b['obs']['lidar'], 'obs_target': b['obs']['target'], 'obs_mask': b['obs']['action_mask'], 'next_lidar': b['next_obs']['lidar'],
               'next_target': b['next_obs']['target'], 'next_mask': b['next_obs']['action_mask'], 'action': b['action'], 'reward': b['reward'],
               'done': b['done'], 'idx': b['idx']}
        for k in want:
            _same(got[k], want[k], k)
        seen.append(ring.counter)
        return inner(b)
    ag.update = update
    out = [tr.step() for _ in range(horizon + 2 * every)]
    assert seen == [1, 2, 3] and tr.updates == 3 and all(np.isfinite(np.array([float(v) for v in o])).all() for o in out if o is not None)
    s = tr.stats()
    assert s['steps'] == horizon + 2 * every and s['episodes'] == int(ring.counts[0]) and math.isfinite(s['mean_reward'])
    e.close()
