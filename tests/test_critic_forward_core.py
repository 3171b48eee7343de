"""The critics' fused forward's rule (hope_amd/csrc/hope_critic_core.h) through its host twin hope_critic_forward_host, on the CPU: its
accuracy against torch's float64 forward next to that of torch's own float32 forward, the policy twin's words without an action
token, the independence of a row from its batch and of a Q from the other rows' actions, the nets critic_shape refuses, the twin's
argument errors, agent_glue.DeviceCritics inside BatchedSAC's and BatchedPPO's updates on a CPU env, and the sanitizer driver of the twin."""
import copy
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import critic_forward_script as S  # noqa: E402
import policy_forward_script as PS  # noqa: E402
from hope_amd import _lib as L  # noqa: E402
from hope_amd import policy as P  # noqa: E402

EINVAL = -1


@pytest.mark.parametrize('kind,t,b', [(k, t, 129) for k, t in S.KINDS] + [('sac', 4, 33), ('sac', 5, 33)])
def test_accuracy_against_torch_float64(kind, t, b):
    """e_twin <= 4 max(e_torch, 2^-22), both measured against the same module in float64 with the image token given: the policy
    forward's bound.  max |Q| is at most 0.33 with these weights and e_torch 1.5 .. 3.4e-7, so the unscaled floor applies."""
    net = S.make_net(kind, t)
    x = S.inputs(b, kind, t)
    got = S.twin(net, x)
    e_torch, e_twin = S.errors(net, x, got)
    print(f'{kind} T={t} b={b}: max |Q| {float(np.abs(got).max()):.3f}, e_torch {e_torch:.3e}, e_twin {e_twin:.3e}, bound {S.bound(e_torch):.3e}')
    assert got.shape == (b,) and np.isfinite(got).all() and e_twin <= S.bound(e_torch), (e_twin, e_torch)
    assert float(np.abs(got).max()) > 1e-3                                                          # not a trivial output


@pytest.mark.parametrize('t', [3, 4])
def test_without_an_action_token_the_words_are_the_policy_twins(t):
    """a critic HopeNet through hope_critic_forward_host and through hope_policy_forward_host(out_dim 1, tanh_out 0): the same words"""
    net = S.make_net('ppo', t)
    x = S.inputs(67, 'ppo', t, seed=2)
    px = dict(x, img_token=None if x['img_token'] is None else np.ascontiguousarray(x['img_token'][0]))
    assert PS.shape_of(net) == (t, 1, 0)
    want = PS.twin(net, px)
    assert np.array_equal(S.words(S.twin(net, x)), S.words(want[:, 0]))


def _rows(x, idx):
    return {k: (None if v is None else np.ascontiguousarray(v[:, idx] if k == 'img_token' else v[idx])) for k, v in x.items()}


@pytest.mark.parametrize('kind,t', S.KINDS)
def test_permuting_the_rows_permutes_the_outputs(kind, t):
    net = S.make_net(kind, t)
    hp = S.host_params(net)
    x = S.inputs(67, kind, t)
    whole = S.twin(net, x, hp)
    perm = np.random.default_rng(5).permutation(67)
    assert np.array_equal(S.words(S.twin(net, _rows(x, perm), hp)), S.words(whole[perm]))
    for i in (0, 1, 31, 32, 33, 66):
        assert np.array_equal(S.words(S.twin(net, _rows(x, slice(i, i + 1)), hp)[0]), S.words(whole[i])), i


@pytest.mark.parametrize('t', [4, 5])
def test_an_action_changes_its_own_row_only(t):
    net = S.make_net('sac', t)
    hp = S.host_params(net)
    x = S.inputs(40, 'sac', t)
    base = S.twin(net, x, hp)
    for i in (0, 1, 33):
        y = dict(x, action=x['action'].copy())
        y['action'][i] = (-0.625, 0.375)
        got = S.twin(net, y, hp)
        differs = S.words(got) != S.words(base)
        assert differs[i] and differs.sum() == 1, (i, np.flatnonzero(differs))


def test_shapes_that_are_refused():
    assert L.critic_shape(S.make_net('ppo', 3)) == (0, 0) and L.critic_shape(S.make_net('ppo', 4)) == (1, 0)
    assert L.critic_shape(S.make_net('sac', 4)) == (0, 1) and L.critic_shape(S.make_net('sac', 5)) == (1, 1)
    with pytest.raises(ValueError, match='output_size = 2'):
        L.critic_shape(P.HopeNet(P.actor_configs(use_img=False)))
    with pytest.raises(ValueError, match='attention trunk'):
        L.critic_shape(P.HopeNet(P.critic_configs(use_img=False, use_attention=False)))
    with pytest.raises(ValueError, match='input_action_dim = 3'):
        L.critic_shape(P.SacCritic(P.critic_configs(use_img=False), 3))
    with pytest.raises(ValueError, match='not Linear'):
        L.critic_shape(torch.nn.Linear(2, 2))
    # policy_shape keeps refusing the action token
    with pytest.raises(ValueError, match='an action token'):
        L.policy_shape(S.make_net('sac', 4).net)


def test_the_twin_refuses_bad_arguments():
    lib = L.load_library()
    for kind, t in (('ppo', 3), ('sac', 5)):
        net = S.make_net(kind, t)
        has_img, has_action = S.flags(kind, t)
        p, keep = S.host_params(net)
        x = S.inputs(3, kind, t)
        tok = None if x['img_token'] is None else np.ascontiguousarray(x['img_token'][0])
        spare_tok, spare_act = np.zeros((3, 128), np.float32), np.zeros((3, 2), np.float32)
        out = np.full((3,), 7.0, np.float32)
        good = dict(p=C.byref(p), has_img=has_img, has_action=has_action, lidar=x['lidar'], target=x['target'], mask=x['mask'], img=tok, action=x['action'],
                    batch=3, out=out)

        def call(**kw):
            a = dict(good, **kw)
            ptr = lambda v: S._p(v) if isinstance(v, np.ndarray) or v is None else v  # noqa: E731
            return lib.hope_critic_forward_host(a['p'], a['has_img'], a['has_action'], *(ptr(a[k]) for k in ('lidar', 'target', 'mask', 'img', 'action')),
                                                a['batch'], ptr(a['out']))

        assert call() == 0 and not (out == 7.0).any()
        out[:] = 7.0
        for k in ('p', 'lidar', 'target', 'mask', 'out'):
            assert call(**{k: None}) == EINVAL and lib.hope_last_error().decode().startswith('hope_critic_forward_host:'), k
        assert call(batch=0) == EINVAL and call(batch=-1) == EINVAL
        assert call(has_img=2) == EINVAL and call(has_action=-1) == EINVAL
        # an image token or an action that does not go with the shape, either way round
        assert call(img=None if has_img else spare_tok) == EINVAL
        assert call(action=None if has_action else spare_act) == EINVAL
        # the action tensors NULL exactly without the action token
        bad = L.CriticParams.from_buffer_copy(p)
        bad.action_w2 = None if has_action else keep[0].ctypes.data
        assert call(p=C.byref(bad)) == EINVAL
        bad = L.CriticParams.from_buffer_copy(p)
        bad.qkv_w = None
        assert call(p=C.byref(bad)) == EINVAL
        assert (out == 7.0).all(), 'a refused call wrote to out'


def _small_env(n=4):
    from fake_env import OracleEnv
    from hope_amd.scenes import SceneSource
    src = SceneSource(levels=('Normal', 'Complex', 'Extrem'), seed=3)
    return OracleEnv([src.draw() for _ in range(n)])


class _Recorder:
    """stands in front of a DeviceCritics and keeps what went through"""

    def __init__(self, inner):
        self.inner, self.calls = inner, []

    def __call__(self, nobs, action=None, which=None):
        out = self.inner(nobs, action, which)
        self.calls.append((nobs, None if action is None else action.clone(), which, out))   # (a DeviceSacUpdate's sample is overwritten by its next)
        return out


def _count_forwards(nets):
    counts = {k: 0 for k in nets}
    for k, m in nets.items():
        m.register_forward_hook(lambda mod, a, o, k=k: counts.__setitem__(k, counts[k] + 1))
    return counts


def test_sac_update_with_device_critics_on_a_cpu_env():
    """_update_with_block with device_critics: every network forward of the plain run but the two target critics', whose values
    come from one DeviceCritics call and equal the twin's word for word; the losses stay within what the forward's rounding allows"""
    from hope_amd import agent_glue as G
    from hope_amd import agents as A
    env = _small_env()
    b = 33
    x, x2 = S.inputs(b, 'sac', 4, seed=1), S.inputs(b, 'sac', 4, seed=2)
    rng = np.random.default_rng(0)
    obs, act = S.nobs(x)
    nobs, _ = S.nobs(x2)
    batch = {'obs': obs, 'next_obs': nobs, 'action': act, 'reward': torch.from_numpy(rng.standard_normal(b).astype(np.float32)),
             'done': torch.from_numpy((rng.random(b) < 0.2).astype(np.float32))}
    noise = (torch.from_numpy(rng.standard_normal((b, 2)).astype(np.float32)), torch.from_numpy(rng.standard_normal((b, 2)).astype(np.float32)))
    runs = {}
    for which in ('plain', 'critics'):
        torch.manual_seed(0)
        ag = A.BatchedSAC(device='cpu', use_img=False, lr=1e-3, update_block=G.DeviceSacUpdate(env))
        for i, m in enumerate((ag.actor, ag.critic1, ag.critic2, ag.critic_target1, ag.critic_target2)):
            S.det_fill(m, salt=0.3 + 0.2 * i)
        counts = _count_forwards({'actor': ag.actor, 'critic1': ag.critic1, 'critic2': ag.critic2, 't1': ag.critic_target1, 't2': ag.critic_target2})
        targets = [copy.deepcopy(ag.critic_target1), copy.deepcopy(ag.critic_target2)]
        if which == 'critics':
            dc = G.make_critics('device', env, ag)
            assert dc is ag.device_critics and not dc.on_device and dc.packs == [0, 0] and dc.shape == (0, 1)
            ag.device_critics = rec = _Recorder(dc)
        losses = ag.update(batch, noise)
        runs[which] = (dict(counts), losses)
        if which == 'critics':
            assert dc.packs == [1, 1] and len(rec.calls) == 1
            seen, na, _, (qt1, qt2) = rec.calls[0]
            assert seen is nobs and qt1.shape == (b, 1) and qt1.dtype == torch.float32
            for q, net in zip((qt1, qt2), targets):
                want = S.twin(net, dict(x2, action=na.numpy()))
                assert np.array_equal(S.words(q.numpy()[:, 0]), S.words(want))
            ag.update(batch, noise)                                  # _soft_update moved both targets: both slots re-pack, once
            assert dc.packs == [2, 2]
    plain, crit = runs['plain'][0], runs['critics'][0]
    assert plain == {'actor': 2, 'critic1': 2, 'critic2': 2, 't1': 1, 't2': 1}, plain
    assert crit == dict(plain, t1=0, t2=0), crit
    assert np.allclose(runs['plain'][1], runs['critics'][1], rtol=1e-4, atol=1e-6), runs
    with pytest.raises(ValueError):
        G.make_critics('gpu', env, ag)
    assert G.make_critics(None, env, ag) is None


class _TwinNet:
    """stands in as a critic module: the host twin on the same observations -> [B, 1]"""

    def __init__(self, net):
        self.net = copy.deepcopy(net)

    def __call__(self, obs):
        x = {'lidar': obs['lidar'].numpy(), 'target': obs['target'].numpy(), 'mask': obs['action_mask'].numpy(), 'img_token': None, 'action': None}
        return torch.from_numpy(S.twin(self.net, {k: (None if v is None else np.ascontiguousarray(v, dtype=np.float32)) for k, v in x.items()})).unsqueeze(1)


@pytest.mark.parametrize('use_gae', [False, True])
def test_ppo_advantages_with_device_critics_on_a_cpu_env(use_gae):
    """BatchedPPO.advantages with device_critics equals, word for word, advantages whose critic and critic_target return the twin's
    values: two DeviceCritics calls (both nets on the block, the critic on last_obs), with the torch advantage block and with DeviceGae"""
    from hope_amd import agent_glue as G
    from hope_amd import agents as A
    env = _small_env()
    n, t = 5, 7
    x, xl = S.inputs(n * t, 'ppo', 3, seed=4), S.inputs(n, 'ppo', 3, seed=6)
    flat, _ = S.nobs(x)
    last, _ = S.nobs(xl)
    obs = {k: v.view((n, t) + v.shape[1:]) for k, v in flat.items()}
    rng = np.random.default_rng(1)
    reward = torch.from_numpy(rng.standard_normal((n, t)).astype(np.float32))
    done = torch.from_numpy((rng.random((n, t)) < 0.15).astype(np.float32))
    torch.manual_seed(0)
    ag = A.BatchedPPO(device='cpu', use_img=False, gae=G.DeviceGae(env) if use_gae else None)
    S.det_fill(ag.critic, salt=0.3)
    S.det_fill(ag.critic_target, salt=0.5)
    dc = G.make_critics('device', env, ag)
    assert dc.nets == [ag.critic, ag.critic_target] and dc.shape == (0, 0)
    ag.device_critics = rec = _Recorder(dc)
    adv, vt = (a.clone() for a in ag.advantages(obs, reward, done, last))
    assert dc.packs == [1, 1] and [c[2] for c in rec.calls] == [None, (0,)]
    ref = A.BatchedPPO(device='cpu', use_img=False, gae=G.DeviceGae(env) if use_gae else None)
    ref.critic, ref.critic_target = _TwinNet(ag.critic), _TwinNet(ag.critic_target)
    adv2, vt2 = ref.advantages(obs, reward, done, last)
    assert np.array_equal(S.words(adv.numpy()), S.words(adv2.numpy())) and np.array_equal(S.words(vt.numpy()), S.words(vt2.numpy()))
    # chunked inputs give the same words
    dc.chunk = 8
    adv3, vt3 = ag.advantages(obs, reward, done, last)
    assert np.array_equal(S.words(adv3.numpy()), S.words(adv.numpy())) and np.array_equal(S.words(vt3.numpy()), S.words(vt.numpy()))
    assert dc.packs == [1, 1]


def test_sanitizer_driver_of_the_twin_runs_clean(tmp_path):
    """tests/critic_forward_host_sanitize.cpp, a stand-alone program, compiled by the host compiler with -fsanitize=address,undefined"""
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / 'critic_forward_host_sanitize')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
           '-I' + os.path.join(root, 'include'), '-I' + os.path.join(root, 'hope_amd', 'csrc'),
           os.path.join(root, 'tests', 'critic_forward_host_sanitize.cpp'), '-o', exe]
    # the runtime linked into the program where the compiler can (gcc's switch; clang does so by default and may not know it)
    if subprocess.run(cmd + ['-static-libasan'], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'clean' in r.stdout, (r.returncode, r.stdout, r.stderr)
