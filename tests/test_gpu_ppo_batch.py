"""k_ppo_gather / k_ppo_loss / k_ppo_merge (hope_amd/csrc/hope_ppo_kernel.h) on the device: word for word their host twins, ordered by
the stream they are enqueued on, misused, and inside PPOTrainer."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_batch_script as S  # noqa: E402

pytestmark = pytest.mark.gpu

N, T = 1030, 4                                        # 4120 transitions
MAX_BATCH = 4097                                      # 65 chunk partials: more than the merge wave has lanes, with an odd one


@pytest.fixture(scope='module')
def env():
    from hope_amd import ParkingBatch
    e = ParkingBatch(N, 32)
    e.enable_ppo_batch(MAX_BATCH)
    yield e
    e.close()


@pytest.fixture(scope='module')
def ring_case():
    return S.ring_arrays(N, T)


def _dev(env, a, offset=0):
    """the array on the device; offset = 1: in a buffer whose base is 4 bytes past the allocation's (only 4-byte aligned)"""
    a = np.ascontiguousarray(a)
    if not offset:
        return torch.from_numpy(a).to(env.device)
    assert a.dtype.itemsize == 4
    buf = torch.zeros(a.size + offset, dtype=torch.from_numpy(a).dtype, device=env.device)
    v = buf[offset:].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 * offset and v.is_contiguous()
    return v


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and np.array_equal(S.words(got), S.words(want)), what


def _ring_on_device(env, r, offset):
    from hope_amd import _lib as L
    t = {k: _dev(env, v, offset) for k, v in r.items()}
    return t, L.ring_desc('test', env.device, N, T, **t)


def _batch_on_device(env, mb, offset, fill=None):
    """the eight tensors of a minibatch (prefilled, or holding `fill`'s arrays) and their descriptor"""
    from hope_amd import _lib as L
    o = S.batch_arrays(mb)
    o.update(fill or {})
    t = {k: _dev(env, v, offset) for k, v in o.items()}
    return t, L.ppo_batch_desc('test', env.device, mb, **t)


def _index(mb, seed=0):
    """a slice of a permutation; from 63 items on with out-of-range rows in it"""
    m = N * T
    index = np.random.default_rng(seed).permutation(m).astype(np.int64)[7:7 + mb].copy()
    if mb >= 63:
        index[[0, 5, 31, mb - 1]] = (-1, m, 2 ** 40, -2 ** 40)
        index[[1, 2]] = (0, m - 1)
    return index


@pytest.mark.parametrize('mb', [1, 63, 64, 65, 129, 4097])
def test_kernels_equal_the_host_twins_word_for_word(env, ring_case, mb):
    """the gather (with refused rows) and the loss from 16-byte aligned bases and from bases 4 bytes past the allocation's: both V forms
    of k_ppo_gather, both load forms of k_ppo_loss"""
    r, adv, vt = ring_case
    index = _index(mb, seed=mb)
    want = S.host_gather(r, adv, vt, index)
    assert mb < 63 or ((want['idx'] == -1).sum() == 4 and not want['lidar'][0].any())
    x = S.loss_inputs(mb)
    want_loss = S.host_loss(x)
    for offset in (0, 1):
        rt, rd = _ring_on_device(env, r, offset)
        ot, od = _batch_on_device(env, mb, offset)
        perm = torch.from_numpy(np.concatenate([np.zeros(3, np.int64), index])).to(env.device)
        env.ppo_gather(rd, _dev(env, adv, offset), _dev(env, vt, offset), perm[3:], od)            # index: a slice view
        for k, w in want.items():
            _same(ot[k], w, (mb, offset, 'gather', k))
        bt, bd = _batch_on_device(env, mb, offset, {k: x[k] for k in ('action', 'old_lp', 'adv', 'v_target')})
        got = env.ppo_loss(_dev(env, x['raw'], offset), _dev(env, x['log_std'], offset), _dev(env, x['value'], offset), bd, mb, S.CLIP)
        assert got is env._ppo_out[mb] and [tuple(g.shape) for g in got] == [(mb, 2), (2,), (mb,), (2,)]
        for g, w, what in zip(got, want_loss, ('g_raw', 'g_log_std', 'g_value', 'losses')):
            _same(g, w, (mb, offset, 'loss', what))
    # outputs that are only 4-byte aligned: the C call with its own buffers
    out = [_dev(env, np.zeros(s, np.float32), 1) for s in ((mb, 2), (2,), (mb,), (2,))]
    P = lambda q: C.c_void_p(q.data_ptr())  # noqa: E731
    bt, bd = _batch_on_device(env, mb, 0, {k: x[k] for k in ('action', 'old_lp', 'adv', 'v_target')})
    ins = [_dev(env, x[k]) for k in ('raw', 'log_std', 'value')]                       # (held: the call sees addresses only)
    rc = env.lib.hope_env_ppo_loss(env.h, *(P(a) for a in ins), bd, mb, S.CLIP, *(P(o) for o in out), env._stream())
    assert rc == 0
    for g, w, what in zip(out, want_loss, ('g_raw', 'g_log_std', 'g_value', 'losses')):
        _same(g, w, (mb, 'offset outputs', what))


def test_the_calls_are_ordered_by_their_stream(env, ring_case):
    """inputs produced by torch on a side stream, both calls enqueued there, the results copied back there: nothing synchronises the
    host in between (the copies to the host wait for that stream only)"""
    from hope_amd import _lib as L
    r, adv, vt = ring_case
    mb = 4097
    index = _index(mb, seed=9)
    x = S.loss_inputs(mb, seed=9)
    side = torch.cuda.Stream(device=env.device)
    pin = lambda a: torch.from_numpy(np.ascontiguousarray(a)).pin_memory()  # noqa: E731
    hr, hx = {k: pin(v) for k, v in r.items()}, {k: pin(v) for k, v in x.items()}
    ha, hv, hi = pin(adv), pin(vt), pin(index)
    ot, od = _batch_on_device(env, mb, 0)
    torch.cuda.synchronize(env.device)
    with torch.cuda.stream(side):
        dr = {k: v.to(env.device, non_blocking=True) for k, v in hr.items()}
        dx = {k: v.to(env.device, non_blocking=True) for k, v in hx.items()}
        da, dv, di = (v.to(env.device, non_blocking=True) for v in (ha, hv, hi))
        for _ in range(40):                                        # some work in front of the values the calls read
            dr = {k: (v * 2.0) * 0.5 for k, v in dr.items()}
            dx = {k: (v * 2.0) * 0.5 for k, v in dx.items()}
        env.ppo_gather(L.ring_desc('test', env.device, N, T, **dr), da, dv, di, od)
        got_gather = {k: v.cpu() for k, v in ot.items()}
        for k in ('action', 'old_lp', 'adv', 'v_target'):
            ot[k].copy_(dx[k])
        got_loss = [g.cpu() for g in env.ppo_loss(dx['raw'], dx['log_std'], dx['value'], od, mb, S.CLIP)]
    for k, w in S.host_gather(r, adv, vt, index).items():
        _same(got_gather[k], w, ('gather', k))
    for g, w, what in zip(got_loss, S.host_loss(x), ('g_raw', 'g_log_std', 'g_value', 'losses')):
        _same(g, w, ('loss', what))
    torch.cuda.synchronize(env.device)


def test_misuse_fails_loudly(ring_case):
    """HOPE_ESTATE before enable; HOPE_EINVAL, each with its text, for a batch of 0 and max_batch + 1, a misaligned index, a NULL field
    of either struct, a NaN clip (and other NULLs and numbers out of range) -- each refused before anything is launched; the handle
    gives the twin's words afterwards; enable, disable, enable again; a re-enable with a larger max_batch"""
    from hope_amd import ParkingBatch
    from hope_amd import _lib as L
    n, t, mb = 70, 4, 100
    e = ParkingBatch(n, 32)
    dev, lib = e.device, e.lib
    r, adv, vt = S.ring_arrays(n, t)
    rt = {k: torch.from_numpy(v).to(dev) for k, v in r.items()}
    da, dv = torch.from_numpy(adv).to(dev), torch.from_numpy(vt).to(dev)
    index = np.random.default_rng(1).integers(0, n * t, size=mb + 2).astype(np.int64)
    di = torch.from_numpy(index).to(dev)
    ot = {k: torch.from_numpy(v).to(dev) for k, v in S.batch_arrays(mb + 1).items()}
    x = S.loss_inputs(mb)
    dx = {k: torch.from_numpy(v).to(dev) for k, v in x.items()}
    gs = [torch.zeros(s, device=dev) for s in ((mb, 2), (2,), (mb,), (2,))]
    P = lambda q: None if q is None else C.c_void_p(q if isinstance(q, int) else q.data_ptr())  # noqa: E731
    err = lambda: lib.hope_last_error().decode()  # noqa: E731

    def gather(batch=mb, ring=True, out=True, adv=da, v_target=dv, index=di, **null):
        rd = L.Ring(n=n, T=t, **{k: (None if k in null else v.data_ptr()) for k, v in rt.items()})
        od = L.PpoBatch(**{k: (None if 'out_' + k in null else v.data_ptr()) for k, v in ot.items()})
        return lib.hope_env_ppo_gather(e.h, rd if ring else None, P(adv), P(v_target), P(index), batch, od if out else None, e._stream())

    def loss(m_=mb, clip=0.2, batch=True, **ptr):
        p = {'raw': dx['raw'], 'log_std': dx['log_std'], 'value': dx['value'], 'g_raw': gs[0], 'g_log_std': gs[1], 'g_value': gs[2], 'losses': gs[3]}
        p.update({k: v for k, v in ptr.items() if k in p})
        bd = L.PpoBatch(**{k: (None if ptr.get(k, 0) is None else dx[k].data_ptr()) for k in ('action', 'old_lp', 'adv', 'v_target')})
        return lib.hope_env_ppo_loss(e.h, P(p['raw']), P(p['log_std']), P(p['value']), bd if batch else None, m_, clip, P(p['g_raw']), P(p['g_log_std']),
                                     P(p['g_value']), P(p['losses']), e._stream())
    assert gather() == -5 and 'hope_env_ppo_gather: the minibatch is off (hope_env_ppo_enable first)' in err()          # HOPE_ESTATE
    assert loss() == -5 and 'hope_env_ppo_loss: the minibatch is off' in err()
    for bad in (0, -1, L.PPO_MAX_BATCH + 1):
        assert lib.hope_env_ppo_enable(e.h, bad) == -1 and 'hope_env_ppo_enable: max_batch must be 1 .. 1048576' in err()
    e.enable_ppo_batch(mb)
    assert gather() == 0 and loss() == 0 and gather(batch=1) == 0 and loss(m_=1) == 0
    for kw, text in (({'batch': 0}, 'batch must be 1 .. max_batch (100)'), ({'batch': mb + 1}, 'batch must be 1 .. max_batch (100)'),
                     ({'index': di.data_ptr() + 4}, 'misaligned buffer (index 8 bytes'), ({'adv': da.data_ptr() + 2}, 'misaligned buffer'),
                     ({'ring': False}, 'null ring'), ({'log_prob': None}, 'null tensor in the ring'), ({'lidar': None}, 'null tensor in the ring'),
                     ({'out': False}, 'null out'), ({'out_idx': None}, 'null tensor in out'), ({'out_old_lp': None}, 'null tensor in out'),
                     ({'adv': None}, 'null adv / v_target / index'), ({'index': None}, 'null adv / v_target / index')):
        assert gather(**kw) == -1 and 'hope_env_ppo_gather: ' in err() and text in err(), (kw, err())                    # HOPE_EINVAL
    for kw, text in (({'m_': 0}, 'mb must be 1 .. max_batch (100)'), ({'m_': mb + 1}, 'mb must be 1 .. max_batch (100)'),
                     ({'clip': float('nan')}, 'clip must be finite and >= 0'), ({'clip': float('inf')}, 'clip must be finite'), ({'clip': -0.5}, 'clip must be'),
                     ({'batch': False}, 'null batch'), ({'old_lp': None}, 'null tensor in batch'), ({'action': None}, 'null tensor in batch'),
                     ({'raw': None}, 'null raw / log_std'), ({'losses': None}, 'null raw / log_std'), ({'g_value': gs[2].data_ptr() + 2}, 'misaligned buffer')):
        assert loss(**kw) == -1 and 'hope_env_ppo_loss: ' in err() and text in err(), (kw, err())

    def words_after(batch):
        """the handle is as usable as before: real calls give the twins' words"""
        od = L.ppo_batch_desc('test', dev, batch, **{k: v[:batch] for k, v in ot.items()})
        e.ppo_gather(L.ring_desc('test', dev, n, t, **rt), da, dv, di[:batch], od)
        for k, w in S.host_gather(r, adv, vt, index[:batch]).items():
            _same(ot[k][:batch], w, ('after', batch, k))
        xb = S.loss_inputs(batch)
        for k in ('action', 'old_lp', 'adv', 'v_target'):
            ot[k][:batch].copy_(torch.from_numpy(xb[k]))
        got = e.ppo_loss(*(torch.from_numpy(xb[k]).to(dev) for k in ('raw', 'log_std', 'value')), od, batch, S.CLIP)
        for g, w, what in zip(got, S.host_loss(xb), ('g_raw', 'g_log_std', 'g_value', 'losses')):
            _same(g, w, ('after', batch, what))
    words_after(mb)
    with pytest.raises(L.HopeError, match='index must be int64'):
        e.ppo_gather(L.ring_desc('test', dev, n, t, **rt), da, dv, di[:mb].int(), L.ppo_batch_desc('test', dev, mb, **{k: v[:mb] for k, v in ot.items()}))
    with pytest.raises(L.HopeError, match='out_desc must be a hope_amd._lib.PpoBatch'):
        e.ppo_gather(L.ring_desc('test', dev, n, t, **rt), da, dv, di[:mb], L.PpoBatch())
    e.disable_ppo_batch()
    assert gather() == -5 and loss() == -5
    e.enable_ppo_batch(mb)
    e.enable_ppo_batch(mb // 2)                                                        # (equal or smaller: nothing changes)
    assert gather() == 0 and gather(batch=mb + 1) == -1
    words_after(mb)
    e.enable_ppo_batch(mb + 1)                                                         # larger: the partials are reallocated
    assert gather(batch=mb + 1) == 0 and gather(batch=mb + 2) == -1
    words_after(mb + 1)
    e.disable_ppo_batch()
    e.disable_ppo_batch()
    e.close()


def test_trainer_with_the_device_minibatch(monkeypatch):
    """PPOTrainer(minibatch='device', gae='device', ring='device'): 256 generated lots, horizon 4, minibatches of 256, two epochs, two
    updates -- finite losses; and one minibatch's seeds, intercepted on their way into torch.autograd.backward, equal the host twin fed
    the very network outputs and gathered tensors the device call was given"""
    from hope_amd import ParkingBatch
    from hope_amd import agent_glue as G
    from hope_amd import agents as A
    from hope_amd.rollout import PPOTrainer
    from hope_amd.scene_gen import mixed_arrays
    n = 256
    arrs = mixed_arrays(n, levels=('Normal', 'Complex', 'Extrem'), seed=11, max_obst=32)
    e = ParkingBatch(n, 32)
    e.set_scene_arrays(np.arange(n), *arrs[:5])
    torch.manual_seed(0)
    ag = A.BatchedPPO(device=e.device, use_img=False, mini_batch=256, mini_epoch=2)
    tr = PPOTrainer(e, ag, horizon=4, seed=2, use_planner='device', gae='device', ring='device', minibatch='device')
    assert isinstance(ag.minibatch, G.DevicePpoBatch) and ag.minibatch.on_device and tr.minibatch is ag.minibatch
    seen = []
    inner = torch.autograd.backward

    def spy(tensors, grad_tensors=None, *a, **kw):
        if grad_tensors is not None and not isinstance(tensors, torch.Tensor) and len(tensors) == 3:
            batch = ag.minibatch._out[256].t
            seen.append(([x.detach().clone() for x in tensors], [g.detach().clone() for g in grad_tensors], {k: v.clone() for k, v in batch.items()},
                         e._ppo_out[256][3].clone()))
        return inner(tensors, grad_tensors, *a, **kw)
    monkeypatch.setattr(torch.autograd, 'backward', spy)
    losses = [x for x in (tr.step() for _ in range(8)) if x is not None]
    monkeypatch.setattr(torch.autograd, 'backward', inner)
    assert tr.updates == 2 and len(losses) == 2 and all(math.isfinite(float(v)) for l_ in losses for v in l_), losses
    assert len(seen) == 2 * 2 * 4                                                      # updates x epochs x minibatches
    for (raw, value, log_std), (g_raw, g_value, g_log_std), batch, dl in (seen[0], seen[5], seen[-1]):
        assert raw.shape == (256, 2) and value.shape == (256, 1) and float(raw.abs().max()) > 0
        idx = batch['idx'].cpu().numpy()
        assert idx.min() >= 0 and idx.max() < n * 4 and len(np.unique(idx)) == 256      # a slice of a permutation
        x = {'raw': raw.cpu().numpy(), 'log_std': log_std.cpu().numpy().reshape(2), 'value': value.cpu().numpy().reshape(-1)}
        x.update({k: batch[k].cpu().numpy() for k in ('action', 'old_lp', 'adv', 'v_target')})
        want = S.host_loss(x, ag.clip)
        assert np.isfinite(want[0]).all() and np.abs(want[0]).max() > 0
        _same(g_raw, want[0], 'g_raw'); _same(g_log_std.view(2), want[1], 'g_log_std'); _same(g_value.view(-1), want[2], 'g_value'); _same(dl, want[3], 'losses')
    batch = seen[-1][2]                                                                # the ring still holds what the last update read
    ri = batch['idx'].long()
    assert torch.equal(batch['action'], tr.ring.action.reshape(-1, 2)[ri]) and torch.equal(batch['lidar'], tr.ring.obs['lidar'].reshape(-1, 120)[ri])
    assert torch.equal(batch['old_lp'], tr.ring.log_prob.reshape(-1, 2).sum(1)[ri])
    assert losses[-1] == tuple(float(v) for v in seen[-1][3].cpu())
    e.close()
