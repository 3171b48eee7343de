"""The rule of PPO's minibatch (hope_amd/csrc/hope_ppo_core.h) through its host twins hope_ppo_gather_host / hope_ppo_loss_host, on the
CPU: the gather against torch's indexing, the loss and its gradients against torch's float64 autograd, the sums' order against a
restatement, BatchedPPO.update with a DevicePpoBatch over CPU tensors, and misuse."""
import copy
import ctypes as C
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_batch_script as S  # noqa: E402

SIZES = (1, 2, 63, 64, 65, 129, 4097)


@pytest.fixture(scope='module')
def loss_case():
    """per size: the inputs, the twin's outputs and the float64 reference, computed once"""
    out = {}
    for mb in SIZES:
        x = S.loss_inputs(mb)
        out[mb] = (x, S.host_loss(x), S.torch_reference(x))
    return out


@pytest.mark.parametrize('n,t', [(1, 1), (3, 5), (70, 4)])
def test_gather_twin_equals_torch_indexing(n, t):
    """the same tensors and index: all eight outputs word for word -- a permutation, repeated entries, a slice view of a permutation at
    an offset; and out-of-range entries (-1, n T, 2^40) give zero rows with idx -1 next to rows that are served"""
    r, adv, vt = S.ring_arrays(n, t)
    m = n * t
    rng = np.random.default_rng(5)
    perm = rng.permutation(m).astype(np.int64)
    mb = max(1, m // 3)
    cases = {'permutation': perm, 'repeated': rng.integers(0, m, size=2 * m + 3).astype(np.int64), 'slice view': perm[m - mb:], 'one': perm[:1]}
    assert cases['slice view'].base is not None
    for name, index in cases.items():
        got, want = S.host_gather(r, adv, vt, index), S.torch_gather(r, adv, vt, index)
        for k in want:
            assert got[k].shape == want[k].shape and np.array_equal(S.words(got[k]), S.words(want[k])), (name, k)
    index = np.concatenate([perm[:2], np.array([-1, m, 2 ** 40, -2 ** 40, 0, m - 1], np.int64)])
    bad = np.array([False] * len(perm[:2]) + [True] * 4 + [False] * 2)
    got, want = S.host_gather(r, adv, vt, index), S.torch_gather(r, adv, vt, index[~bad])
    for k in want:
        assert np.array_equal(S.words(got[k][~bad]), S.words(want[k])), k
        if k != 'idx':
            assert not S.words(got[k][bad]).any(), k                           # +0.0, every word
    assert (got['idx'][bad] == -1).all()


@pytest.mark.parametrize('mb', SIZES)
def test_loss_twin_against_float64_autograd(loss_case, mb):
    """g_raw and g_value per item within one float32 ulp of the float64 reference; g_log_std and the two losses within one ulp plus
    2^-40 sum |terms| (float64 arithmetic rounded once: the reference's own sums run in another order).  From 63 items on the inputs
    hold every branch of the rule, which is asserted."""
    x, (g_raw, g_log_std, g_value, losses), ref = loss_case[mb]
    if mb >= 63:
        cs = S.census(x, ref)
        assert min(cs.values()) > 0, cs
        assert (ref['u'] == ref['c']).sum() >= (x['adv'] == 0).sum() > 0       # ties of the min: unclipped ratios and a == 0
    for got, want, what in ((g_raw, ref['g_raw'], 'g_raw'), (g_value, ref['g_value'], 'g_value')):
        err = np.abs(got.astype(np.float64) - want)
        print(mb, what, 'largest error in ulp:', float((err / S.ulp32(want)).max()))
        assert got.shape == want.shape and (err <= S.ulp32(want)).all(), (what, float((err / S.ulp32(want)).max()))
    assert not g_raw[np.abs(x['raw']) > 1].any()                                # beyond the clamp: no gradient
    if mb >= 63:                                                                # exactly on the clamp's bounds: the gradient passes
        assert g_raw[np.abs(x['raw']) == 1].any() and ref['g_raw'][np.abs(x['raw']) == 1].any()
    for got, want, slack, what in ((g_log_std, ref['g_log_std'], ref['abs_sums'][2:], 'g_log_std'), (losses, ref['losses'], ref['abs_sums'][:2], 'losses')):
        err, bound = np.abs(got.astype(np.float64) - want), S.ulp32(want) + 2.0 ** -40 * slack
        print(mb, what, 'error / bound:', (err / np.maximum(bound, 1e-300)).tolist())
        assert (err <= bound).all(), (what, err, bound)


def test_the_sums_have_the_rules_order(loss_case):
    """4097 items (65 chunk partials, an odd one among them) in one call of the twin, against the script's own restatement: the
    per-item terms in Python floats, the chunk tree, the merge tree -- equal word for word"""
    x, (_, g_log_std, _, losses), _ = loss_case[4097]
    want_g, want_l = S.restated_sums(x)
    assert np.array_equal(S.words(g_log_std), S.words(want_g)), (g_log_std, want_g)
    assert np.array_equal(S.words(losses), S.words(want_l)), (losses, want_l)


def _ring_and_agent(n=6, t=4, mini_batch=10, seed=0, **kw):
    """a full CPU TransitionRing with drawn contents, a BatchedPPO over it and given advantages"""
    from hope_amd import agents as A
    from hope_amd.rollout import TransitionRing
    torch.manual_seed(seed)
    ring = TransitionRing(n, t, ('lidar', 'target', 'action_mask'), 'cpu')
    for v in ring.obs.values():
        v.copy_(torch.randn(v.shape))
    ring.obs['action_mask'].copy_((torch.rand(n, t, 42) > 0.3).float())
    ring.action.copy_(torch.randn(n, t, 2).clamp(-1, 1))
    ring.log_prob.copy_(-1.0 + 0.3 * torch.randn(n, t, 2))
    ring.reward.copy_(torch.randn(n, t))
    ring.head, ring.size = 0, t
    ag = A.BatchedPPO(device='cpu', use_img=False, lr=0.0, mini_batch=mini_batch, mini_epoch=1, state_norm=False, **kw)
    with torch.no_grad():
        ag.log_std.copy_(torch.tensor([[-0.2, 0.1]]))
    adv, v_target = torch.randn(n, t), torch.randn(n, t)
    adv[0, 0] = 0.0
    last = {k: v[:, 0].clone() for k, v in ring.obs.items()}
    return ring, ag, adv, v_target, last


def _update(ag, ring, adv, v_target, last, perms, dtype=torch.float32):
    ag.advantages = lambda *a, **k: (adv.to(dtype), v_target.to(dtype))        # the minibatch loop alone: the same advantages for every path
    obs, action, reward, done, log_prob = ring.ordered()
    if dtype != torch.float32:
        obs, action, reward, done, log_prob, last = ({k: v.to(dtype) for k, v in obs.items()}, action.to(dtype), reward.to(dtype), done.to(dtype),
                                                     log_prob.to(dtype), {k: v.to(dtype) for k, v in last.items()})
    return ag.update(obs, action, reward, done, log_prob, last, perms=perms)


def test_update_with_the_device_minibatch_on_cpu_tensors(monkeypatch):
    """BatchedPPO.update(minibatch=DevicePpoBatch) over a CPU ring, perms given, learning rate 0 (every minibatch sees the same
    weights): the seeds handed to torch.autograd.backward equal the twin's words for the very raw and value the call was given; the
    parameter gradients of the last minibatch are at most 2 x as far from the float64 torch path as the float32 torch path is (both
    push float32 seeds through the same float32 backward and differ in the seeds' last bits only), per parameter tensor"""
    from hope_amd import agent_glue as G
    ring, ag, adv, v_target, last = _ring_and_agent()
    m = ring.n * ring.T
    perms = [torch.randperm(m, generator=torch.Generator().manual_seed(3))]
    ag32, ag64 = copy.deepcopy(ag), copy.deepcopy(ag)
    ag64.actor.double(); ag64.critic.double(); ag64.critic_target.double()
    ag64.log_std.data = ag64.log_std.data.double()
    env = types.SimpleNamespace(n=ring.n, device=torch.device('cpu'))
    ag.minibatch = G.make_ppo_batch('device', env, ring)
    assert isinstance(ag.minibatch, G.DevicePpoBatch) and not ag.minibatch.on_device and G.make_ppo_batch(None, env, ring) is None
    with pytest.raises(ValueError):
        G.make_ppo_batch('gpu', env, ring)
    seen = []
    inner = torch.autograd.backward

    def spy(tensors, grad_tensors=None, *a, **kw):
        if grad_tensors is not None and not isinstance(tensors, torch.Tensor) and len(tensors) == 3:
            seen.append(([x.detach().clone() for x in tensors], [g.detach().clone() for g in grad_tensors]))
        return inner(tensors, grad_tensors, *a, **kw)
    monkeypatch.setattr(torch.autograd, 'backward', spy)
    got = _update(ag, ring, adv, v_target, last, perms)
    monkeypatch.setattr(torch.autograd, 'backward', inner)
    assert len(seen) == 3 and [s[0][0].shape[0] for s in seen] == [10, 10, 4]           # 24 transitions in minibatches of 10
    flat = lambda v: v.reshape((m,) + v.shape[2:]).numpy()  # noqa: E731
    for k, ((raw, value, log_std), (g_raw, g_value, g_log_std)) in enumerate(seen):
        ri = perms[0][10 * k:10 * k + 10].numpy()
        x = {'raw': raw.numpy(), 'log_std': log_std.numpy().reshape(2), 'value': value.numpy().reshape(-1), 'action': flat(ring.action)[ri],
             'old_lp': flat(ring.log_prob.sum(2))[ri], 'adv': flat(adv)[ri], 'v_target': flat(v_target)[ri]}
        want = S.host_loss(x, ag.clip)
        assert g_raw.shape == raw.shape and g_value.shape == value.shape == (len(ri), 1) and g_log_std.shape == (1, 2)
        for a, b, what in ((g_raw, want[0], 'g_raw'), (g_log_std, want[1], 'g_log_std'), (g_value, want[2], 'g_value')):
            assert np.array_equal(S.words(a.numpy().reshape(b.shape)), S.words(b)), (k, what)
    assert np.array_equal(S.words(np.array(got, np.float32)), S.words(want[3]))         # last_losses: the last minibatch's
    l32 = _update(ag32, ring, adv, v_target, last, perms)
    l64 = _update(ag64, ring, adv, v_target, last, perms, torch.float64)
    assert max(abs(a - b) for a, b in zip(got, l64)) <= 1e-6 * max(1.0, *map(abs, l64)) and max(abs(a - b) for a, b in zip(l32, l64)) <= 1e-5
    worst, compared = 0.0, 0
    for (name, p), p32, p64 in zip([(n_, p) for n_, p in list(ag.actor.named_parameters()) + [('log_std', ag.log_std)] + list(ag.critic.named_parameters())],
                                   ag32.trainable(), ag64.trainable()):
        if p64.grad is None:                                                    # a parameter the forward without the image does not use
            assert p.grad is None and p32.grad is None, name
            continue
        assert p.grad is not None and p.grad.shape == p64.grad.shape, name
        compared += 1
        yard = float((p32.grad.double() - p64.grad).abs().max())
        dist = float((p.grad.double() - p64.grad).abs().max())
        worst = max(worst, dist / yard if yard > 0 else (0.0 if dist == 0 else float('inf')))
        assert dist <= 2.0 * yard, (name, dist, yard)
    assert compared > 20
    print('largest distance / yardstick over the', compared, 'parameter tensors:', worst)


def test_update_without_a_minibatch_is_todays_path():
    """minibatch=None: the losses and every parameter after an update with a real learning rate equal, bit for bit, those of the loop
    as it was before the switch (restated in the script), from the same seed; a ring that is not full from column 0, or other
    tensors than the ring's, are refused by the device minibatch"""
    from hope_amd import agent_glue as G
    ring, ag, adv, v_target, last = _ring_and_agent(seed=1)
    for opt in (ag.actor_opt, ag.critic_opt):
        for g in opt.param_groups:
            g['lr'] = 1e-3
    ag.mini_epoch = 2
    assert ag.minibatch is None
    m = ring.n * ring.T
    perms = [torch.randperm(m, generator=torch.Generator().manual_seed(s)) for s in (4, 5)]
    twin = copy.deepcopy(ag)
    got = _update(ag, ring, adv, v_target, last, perms)
    twin.advantages = lambda *a, **k: (adv, v_target)
    want = S.parent_update(twin, *ring.ordered(), last, perms)
    assert got == want and ag.last_losses == want
    for p, q in zip(ag.trainable() + list(ag.critic_target.parameters()), twin.trainable() + list(twin.critic_target.parameters())):
        assert torch.equal(p, q)
    env = types.SimpleNamespace(n=ring.n, device=torch.device('cpu'))
    ag.minibatch = G.DevicePpoBatch(env, ring)
    obs, action, reward, done, log_prob = ring.ordered()
    with pytest.raises(ValueError, match='other tensors'):
        ag.update(obs, action.clone(), reward, done, log_prob, last, perms=perms)
    ring.head, ring.size = 1, ring.T
    with pytest.raises(ValueError, match='full ring'):
        ag.minibatch.gather(adv, v_target, perms[0][:4])


def test_misuse_of_the_host_twins():
    """HOPE_EINVAL with the call's name for a NULL pointer, mb or batch < 1 and a clip that is NaN, negative or infinite; the binding's
    checker refuses a wrong tensor before the call"""
    from hope_amd import _lib as L
    from hope_amd import agent_glue as G
    lib = L.load_library()
    x = S.loss_inputs(5)
    out = [np.zeros(s, np.float32) for s in ((5, 2), (2,), (5,), (2,))]
    names = ('raw', 'log_std', 'value', 'g_raw', 'g_log_std', 'g_value', 'losses')
    fields = ('action', 'old_lp', 'adv', 'v_target')

    def loss(mb=5, clip=0.2, batch=True, **null):
        p = dict(zip(names, [x['raw'], x['log_std'], x['value']] + out))
        q = [None if k in null else C.c_void_p(p[k].ctypes.data) for k in names]
        b = L.PpoBatch(**{k: x[k].ctypes.data for k in fields if k not in null}) if batch else None
        return lib.hope_ppo_loss_host(*q[:3], b, mb, clip, *q[3:])
    assert loss() == 0
    for kw in [{'mb': 0}, {'mb': -4}, {'clip': float('nan')}, {'clip': -0.1}, {'clip': float('inf')}, {'batch': False}] + \
            [{k: None} for k in names + fields]:
        assert loss(**kw) == -1 and b'hope_ppo_loss_host' in lib.hope_last_error(), kw
    r, adv, vt = S.ring_arrays(3, 5)
    index = np.arange(4, dtype=np.int64)
    o = S.batch_arrays(4)

    def gather(batch=4, ring=True, out=True, **null):
        rs = S.ring_struct(r)
        for k in null:
            if hasattr(rs, k):
                setattr(rs, k, None)
        os_ = L.PpoBatch(**{k: v.ctypes.data for k, v in o.items() if 'out_' + k not in null})
        P = lambda a, k: None if k in null else C.c_void_p(a.ctypes.data)  # noqa: E731
        return lib.hope_ppo_gather_host(rs if ring else None, P(adv, 'adv'), P(vt, 'v_target'), P(index, 'index'), batch, os_ if out else None)
    assert gather() == 0
    for kw in [{'batch': 0}, {'batch': -1}, {'ring': False}, {'out': False}, {'adv': None}, {'v_target': None}, {'index': None}, {'log_prob': None},
               {'lidar': None}, {'out_idx': None}, {'out_old_lp': None}]:
        assert gather(**kw) == -1 and b'hope_ppo_gather_host' in lib.hope_last_error(), kw
    ring, ag, adv_t, vt_t, _ = _ring_and_agent()
    mbt = G.DevicePpoBatch(types.SimpleNamespace(n=ring.n, device=torch.device('cpu')), ring)
    with pytest.raises(L.HopeError, match=r'hope_ppo_gather_host: adv must be float32 \[24\]'):
        mbt.gather(adv_t[:5], vt_t, torch.arange(4))
    st, batch = mbt.gather(adv_t, vt_t, torch.arange(4))
    assert set(st) == {'lidar', 'target', 'action_mask'} and batch.mb == 4
    with pytest.raises(L.HopeError, match=r'hope_ppo_loss_host: raw must be float32 \[4, 2\]'):
        mbt.backward(torch.zeros(3, 2, requires_grad=True), torch.zeros(4, 1, requires_grad=True), ag.log_std, batch, 0.2)


# ---- the sanitizer driver of the twins -----------------------------------------------------------------------------------------
def test_sanitizer_driver_of_the_twins_runs_clean(tmp_path):
    """tests/ppo_batch_host_sanitize.cpp, a stand-alone program, compiled by the host compiler with -fsanitize=address,undefined"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'ppo_batch_host_sanitize')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
           '-I' + os.path.join(root, 'include'), '-I' + os.path.join(root, 'hope_amd', 'csrc'), os.path.join(root, 'tests', 'ppo_batch_host_sanitize.cpp'),
           '-o', exe]
    # the runtime linked into the program where the compiler can (gcc's switch; clang does so by default and may not know it)
    if subprocess.run(cmd + ['-static-libasan'], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'clean' in r.stdout, (r.returncode, r.stdout, r.stderr)
