"""k_gae_scan / k_gae_merge / k_adv_apply (hope_amd/csrc/hope_gae_kernel.h) on the device: word for word their host twins, ordered by
the stream they are enqueued on, misused, and inside PPOTrainer."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gae_script as GS  # noqa: E402

pytestmark = pytest.mark.gpu

N = 4097                                              # 65 chunks: more partials than the merge wave has lanes, with an odd one
TS = (1, 2, 5, 16, 17)                                # 16: four time steps per load; the others one


@pytest.fixture(scope='module')
def env():
    from hope_amd import ParkingBatch
    e = ParkingBatch(N, 32)
    e.enable_gae()
    yield e
    e.close()


def _dev(env, a, offset=0):
    """the array on the device; offset = 1: in a buffer whose base is 4 bytes past the allocation's (only 4-byte aligned)"""
    a = np.ascontiguousarray(a)
    if not offset:
        return torch.from_numpy(a).to(env.device)
    buf = torch.zeros(a.size + offset, dtype=torch.float32, device=env.device)
    v = buf[offset:].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 * offset and v.is_contiguous()
    return v


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and np.array_equal(GS.words(got), GS.words(want)), what


@pytest.mark.parametrize('rows', [1, 63, 64, 65, 129, 4097])
def test_kernels_equal_the_host_twins_word_for_word(env, rows):
    """per T and done pattern: the fused call (adv normalised in place, v_target, sums as uint64 words), the split call (plain adv and
    sums, then adv_normalize into another tensor and onto adv itself), the scan alone, and the same from bases that are only 4-byte
    aligned (inputs through ParkingBatch.gae, outputs through the C call)"""
    from hope_amd import _lib as L
    for t in TS:
        for pat in GS.PATTERNS:
            x = GS.inputs(rows, t, pat)
            plain, v_target, sums, _ = GS.host_gae(*x, flags=L.GAE_SUMS, delta=False)
            normed = GS.host_normalize(plain, sums)
            what = (rows, t, pat)
            for offset in (0, 1):
                d = [_dev(env, a, offset) for a in x]
                adv, vt, s = env.gae(*d, GS.GAMMA, GS.LAM)                                   # fused
                assert s is env.gae_sums and adv.shape == (rows, t) and adv.is_contiguous()
                _same(adv, normed, what + ('fused adv', offset)); _same(vt, v_target, what + ('v_target', offset)); _same(s, sums, what + ('sums', offset))
                own = torch.full((3,), -1.0, dtype=torch.float64, device=env.device)
                adv, vt, s = env.gae(*d, GS.GAMMA, GS.LAM, normalize=False, sums=own)        # split
                assert s is own
                _same(adv, plain, what + ('plain adv', offset)); _same(vt, v_target, what); _same(own, sums, what + ('own sums', offset))
                out = torch.full((rows, t), 7.0, device=env.device)
                assert env.adv_normalize(adv, own, out=out) is out
                _same(out, normed, what + ('split', offset)); _same(adv, plain, what + ('adv kept', offset))
                assert env.adv_normalize(adv, own) is adv                                    # out aliases adv
                _same(adv, normed, what + ('in place', offset))
            own.fill_(-1.0)
            adv, vt, _ = env.gae(*d, GS.GAMMA, GS.LAM, normalize=None, sums=own)             # the scan alone: no sums
            _same(adv, plain, what + ('scan',)); _same(own, np.full(3, -1.0), what + ('untouched sums',))
    # outputs and sums that are only 4-byte / 8-byte aligned: the C call with its own buffers (last shape of the loop, T = 17, and T = 16)
    for t in (16, 17):
        x = GS.inputs(rows, t, 'random', seed=1)
        plain, v_target, sums, _ = GS.host_gae(*x, flags=L.GAE_NORMALIZE, delta=False)
        d = [_dev(env, a) for a in x]
        oa, ov = (_dev(env, np.zeros((rows, t), np.float32), 1) for _ in range(2))
        sb = torch.zeros(4, dtype=torch.float64, device=env.device)
        P = lambda q: C.c_void_p(q.data_ptr())  # noqa: E731
        rc = env.lib.hope_env_gae(env.h, *(P(a) for a in d), rows, t, GS.GAMMA, GS.LAM, L.GAE_NORMALIZE, P(oa), P(ov), P(sb[1:]), env._stream())
        assert rc == 0
        _same(oa, plain, (rows, t, 'offset outputs')); _same(ov, v_target, (rows, t)); _same(sb[1:], sums, (rows, t))


def test_the_call_is_ordered_by_its_stream(env):
    """inputs produced by torch on a side stream, the call enqueued there, the results copied back there: nothing synchronises the
    host in between (the copies to the host wait for that stream only)"""
    rows, t = 4097, 16
    x = GS.inputs(rows, t, 'random', seed=2)
    side = torch.cuda.Stream(device=env.device)
    host = [torch.from_numpy(a).pin_memory() for a in x]
    torch.cuda.synchronize(env.device)
    with torch.cuda.stream(side):
        d = [h.to(env.device, non_blocking=True) for h in host]
        for _ in range(40):                                        # some work in front of the values the call reads
            d = [(a * 2.0) * 0.5 for a in d]
        adv, vt, s = env.gae(*d, GS.GAMMA, GS.LAM)
        got = [q.cpu() for q in (adv, vt, s)]
    plain, v_target, sums, _ = GS.host_gae(*x, flags=GS.L.GAE_SUMS, delta=False)
    _same(got[0], GS.host_normalize(plain, sums), 'adv'); _same(got[1], v_target, 'v_target'); _same(got[2], sums, 'sums')
    torch.cuda.synchronize(env.device)


def test_misuse_fails_loudly():
    """HOPE_ESTATE before enable; HOPE_EINVAL for rows of 0 and N + 1, T of 0 and 4097, a NULL v_last (and other NULLs, a misaligned
    pointer, an unknown flag, a NaN gamma) -- each with its text, each refused before anything is launched; the handle works
    afterwards; enable, disable, enable again"""
    from hope_amd import ParkingBatch
    from hope_amd import _lib as L
    n, t = 70, 4
    e = ParkingBatch(n, 32)
    dev, lib = e.device, e.lib
    big = [torch.zeros((n + 1) * t + 1, device=dev) for _ in range(7)]
    names = ('reward', 'done', 'value', 'v_last', 'value_target', 'adv', 'v_target')
    sums = torch.zeros(3, dtype=torch.float64, device=dev)

    def raw(rows=n, T=t, gamma=0.98, lam=0.95, flags=L.GAE_NORMALIZE, sums=sums, **ptr):
        p = {k: b.data_ptr() for k, b in zip(names, big)}
        p.update(ptr)
        q = [C.c_void_p(p[k]) if p[k] is not None else None for k in names]
        return lib.hope_env_gae(e.h, *q[:5], rows, T, gamma, lam, flags, q[5], q[6], C.c_void_p(sums.data_ptr()) if sums is not None else None,
                                e._stream())

    def norm(adv=big[5], count=n * t, sums=sums, out=big[5]):
        P = lambda q: None if q is None else C.c_void_p(q.data_ptr())  # noqa: E731
        return lib.hope_env_adv_normalize(e.h, P(adv), count, P(sums), P(out), e._stream())
    err = lambda: lib.hope_last_error().decode()  # noqa: E731
    assert raw() == -5 and 'hope_env_gae: the advantage block is off (hope_env_gae_enable first)' in err()             # HOPE_ESTATE
    assert norm() == -5 and 'hope_env_adv_normalize: the advantage block is off' in err()
    with pytest.raises(L.HopeError, match='code -5'):
        e.gae(*(torch.zeros((n, t), device=dev) for _ in range(3)), torch.zeros(n, device=dev), torch.zeros((n, t), device=dev), 0.98, 0.95)
    e.enable_gae()
    assert raw() == 0 and raw(sums=None) == 0 and raw(flags=0) == 0 and raw(rows=1, T=1) == 0
    for kw, text in (({'rows': 0}, 'rows must be 1 .. the handle'), ({'rows': n + 1}, 'rows must be 1 .. the handle'), ({'rows': -3}, 'rows must be'),
                     ({'T': 0}, 'T must be 1 .. 4096'), ({'T': 4097}, 'T must be 1 .. 4096'), ({'v_last': None}, 'null reward / done / value / v_last'),
                     ({'reward': None}, 'null reward'), ({'adv': None}, 'null reward'), ({'v_target': None}, 'null reward'),
                     ({'value': big[2].data_ptr() + 2}, 'misaligned buffer'), ({'sums': sums.view(torch.float32)[1:]}, 'misaligned buffer'),
                     ({'flags': 4}, 'flags are HOPE_GAE_SUMS'), ({'gamma': float('nan')}, 'not finite'), ({'lam': float('-inf')}, 'not finite')):
        assert raw(**kw) == -1 and 'hope_env_gae: ' in err() and text in err(), (kw, err())                             # HOPE_EINVAL
    for kw, text in (({'adv': None}, 'null adv / out'), ({'out': None}, 'null adv / out'), ({'count': 0}, 'count must be'),
                     ({'count': n * 4096 + 1}, 'count must be'), ({'sums': sums.view(torch.float32)[1:]}, 'misaligned')):
        assert norm(**kw) == -1 and 'hope_env_adv_normalize: ' in err() and text in err(), (kw, err())
    # the handle is as usable as before: a real call gives the twin's words
    x = GS.inputs(n, t, 'random', seed=4)
    adv, vt, s = e.gae(*(torch.from_numpy(a).to(dev) for a in x), GS.GAMMA, GS.LAM)
    plain, v_target, hs, _ = GS.host_gae(*x, flags=L.GAE_SUMS, delta=False)
    _same(adv, GS.host_normalize(plain, hs), 'after the refusals'); _same(vt, v_target, 'v_target'); _same(s, hs, 'sums')
    for bad in (dict(reward=torch.zeros((n, t), device=dev).double()), dict(v_last=torch.zeros((n, 1), device=dev)),
                dict(done=torch.zeros((t, n), device=dev).t()), dict(value=torch.zeros((n, t)))):
        args = dict(reward=torch.zeros((n, t), device=dev), done=torch.zeros((n, t), device=dev), value=torch.zeros((n, t), device=dev),
                    v_last=torch.zeros(n, device=dev), value_target=torch.zeros((n, t), device=dev))
        args.update(bad)
        with pytest.raises(L.HopeError):
            e.gae(gamma=0.98, lam=0.95, **args)
    e.disable_gae()
    assert raw() == -5 and norm() == -5
    e.enable_gae()
    e.enable_gae()                                                                     # (idempotent)
    assert raw() == 0 and norm() == 0
    adv, vt, s = e.gae(*(torch.from_numpy(a).to(dev) for a in x), GS.GAMMA, GS.LAM)
    _same(adv, GS.host_normalize(plain, hs), 'enabled again')
    e.disable_gae()
    e.disable_gae()
    e.close()


def test_trainer_with_the_device_block():
    """PPOTrainer(gae='device'): 256 generated lots, horizon 4, two updates -- finite losses; and `advantages` on the ring's last
    contents equals the host twins fed the very critic outputs the device call was given, with and without the normalisation"""
    from hope_amd import ParkingBatch
    from hope_amd import agent_glue as G
    from hope_amd import agents as A
    from hope_amd import _lib as L
    from hope_amd.rollout import PPOTrainer
    from hope_amd.scene_gen import mixed_arrays
    n = 256
    arrs = mixed_arrays(n, levels=('Normal', 'Complex', 'Extrem'), seed=11, max_obst=32)
    e = ParkingBatch(n, 32)
    e.set_scene_arrays(np.arange(n), *arrs[:5])
    torch.manual_seed(0)
    ag = A.BatchedPPO(device=e.device, use_img=False, mini_batch=n * 4, mini_epoch=1)
    tr = PPOTrainer(e, ag, horizon=4, seed=2, use_planner='device', gae='device')
    assert isinstance(ag.gae, G.DeviceGae) and ag.gae.on_device and tr.gae is ag.gae
    losses = [x for x in (tr.step() for _ in range(8)) if x is not None]
    assert tr.updates == 2 and len(losses) == 2 and all(math.isfinite(float(v)) for l_ in losses for v in l_), losses
    assert float(ag.gae.sums[2]) == n * 4
    for _ in range(4):
        tr.collect_step()
    obs, _, reward, done, _ = tr.ring.ordered()
    seen = {}
    inner = ag.gae

    def spy(*a, **kw):
        seen['x'] = [q.detach().float().cpu().numpy().copy() for q in a[:5]]
        return inner(*a, **kw)
    for adv_norm in (True, False):
        ag.gae, ag.adv_norm = spy, adv_norm
        adv, vt = ag.advantages(obs, reward, done, tr.last_obs())
        want_adv, want_vt, _, _ = GS.host_gae(*seen['x'], ag.gamma, ag.lam, flags=L.GAE_NORMALIZE if adv_norm else 0, delta=False)
        assert np.abs(seen['x'][2]).max() > 0 and np.isfinite(want_adv).all()
        _same(adv, want_adv, ('advantages', adv_norm)); _same(vt, want_vt, ('v_target', adv_norm))
    e.close()
