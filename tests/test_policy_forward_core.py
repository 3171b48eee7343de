"""The fused policy forward's rule (hope_amd/csrc/hope_policy_core.h) through its host twin hope_policy_forward_host, on the CPU: its
accuracy against torch's float64 forward next to that of torch's own float32 forward, the independence of a row from its batch,
agent_glue.DeviceActor on a CPU env (re-pack after an optimiser step and a load_state_dict, none without a change), the nets it
refuses, and the sanitizer driver of the twin."""
import copy
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_forward_script as S  # noqa: E402

CPU_ENV = types.SimpleNamespace(n=1, device=torch.device('cpu'))


@pytest.mark.parametrize('kind,t', S.KINDS)
def test_accuracy_against_torch_float64(kind, t):
    """e_twin <= 4 max(e_torch, 2^-22) at B = 257, both measured against the same module in float64 (DESIGN 5m records them)"""
    net = S.make_net(kind, t)
    x = S.inputs(257, t)
    assert (x['mask'].sum(1) == 0).any() and (np.abs(x['lidar']) == 10).any() and (np.abs(x['target']) == 10).any()
    got = S.twin(net, x)
    e_torch, e_twin = S.errors(net, x, got)
    print(f'{kind} T={t}: e_torch {e_torch:.3e}, e_twin {e_twin:.3e}, bound {S.bound(e_torch):.3e}')
    assert np.isfinite(got).all() and e_twin <= S.bound(e_torch), (e_twin, e_torch)
    assert got.shape == (257, 2 if kind == 'actor' else 1) and float(np.abs(got).max()) > 1e-3        # not a trivial output


@pytest.mark.parametrize('t', [3, 4])
def test_a_row_does_not_depend_on_its_batch(t):
    """row i of a B = 129 call equals, word for word, the B = 1 call on row i (16 rows) and the same row after the batch is reversed"""
    net = S.make_net('actor', t)
    hp = S.host_params(net)
    x = S.inputs(129, t)
    whole = S.twin(net, x, hp)
    rev = S.twin(net, {k: (None if v is None else np.ascontiguousarray(v[::-1])) for k, v in x.items()}, hp)
    assert np.array_equal(S.words(rev[::-1]), S.words(whole))
    for i in (0, 1, 2, 17, 31, 32, 33, 34, 63, 64, 65, 95, 96, 97, 127, 128):
        one = S.twin(net, {k: (None if v is None else np.ascontiguousarray(v[i:i + 1])) for k, v in x.items()}, hp)
        assert np.array_equal(S.words(one[0]), S.words(whole[i])), i


def _nobs(x):
    return {'lidar': torch.from_numpy(x['lidar']), 'target': torch.from_numpy(x['target']), 'action_mask': torch.from_numpy(x['mask'])}


def test_device_actor_on_a_cpu_env():
    """matches policy_mean within the accuracy test's bound; after an Adam step on the actor, and after a load_state_dict, the next
    call equals a fresh twin call on the new weights word for word; with nothing changed no second pack happens"""
    from hope_amd import agent_glue as G
    from hope_amd import agents as A
    torch.manual_seed(0)
    ag = A.BatchedPPO(device='cpu', use_img=False)
    S.det_fill(ag.actor, salt=0.25)
    x = S.inputs(65, 3, seed=5)
    nobs = _nobs(x)
    plain = ag.policy_mean(nobs).numpy()
    actor = G.make_actor('device', CPU_ENV, ag)
    assert actor is ag.device_actor and not actor.on_device and actor.packs == 0
    got = ag.policy_mean(nobs).numpy()
    assert actor.packs == 1
    ref = torch.clamp(copy.deepcopy(ag.actor).double()({k: v.double() for k, v in nobs.items()}), -1, 1).detach().numpy()
    e_torch, e_dev = float(np.abs(plain - ref).max()), float(np.abs(got - ref).max())
    assert e_dev <= S.bound(e_torch), (e_dev, e_torch)
    assert np.array_equal(S.words(got), S.words(np.clip(S.twin(ag.actor, x), -1, 1)))
    again = ag.policy_mean(nobs).numpy()
    assert actor.packs == 1 and np.array_equal(S.words(again), S.words(got))                  # nothing changed: no pack
    # an in-place optimiser step
    loss = ag.actor(nobs).square().sum()
    ag.actor_opt.zero_grad()
    loss.backward()
    for g in ag.actor_opt.param_groups:
        g['lr'] = 1e-3
    ag.actor_opt.step()
    stepped = ag.policy_mean(nobs).numpy()
    assert actor.packs == 2 and not np.array_equal(S.words(stepped), S.words(got))
    assert np.array_equal(S.words(stepped), S.words(np.clip(S.twin(ag.actor, x), -1, 1)))
    # load_state_dict
    ag.actor.load_state_dict(S.make_net('actor', 3).state_dict())
    loaded = ag.policy_mean(nobs).numpy()
    assert actor.packs == 3
    assert np.array_equal(S.words(loaded), S.words(np.clip(S.twin(S.make_net('actor', 3), x), -1, 1)))
    assert ag.policy_mean(nobs) is not None and actor.packs == 3
    # the default path is untouched once the actor is taken away again
    ag.device_actor = None
    assert np.array_equal(ag.policy_mean(nobs).numpy(), torch.clamp(ag.actor(nobs), -1, 1).detach().numpy())
    with pytest.raises(ValueError, match="None or 'device'"):
        G.make_actor('gpu', CPU_ENV, ag)


def test_device_actor_with_an_image():
    """use_img: the image encoder runs in torch, its token goes to the twin ready-made"""
    from hope_amd import agent_glue as G
    net = S.make_net('actor', 4)
    x = S.inputs(9, 4)
    nobs = _nobs(x)
    nobs['img'] = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (9, 3, 64, 64), dtype=np.uint8))
    got = G.DeviceActor(CPU_ENV, net)(nobs).numpy()
    with torch.no_grad():
        ref = torch.clamp(copy.deepcopy(net).double()({k: (v if v.dtype == torch.uint8 else v.double()) for k, v in nobs.items()}), -1, 1).numpy()
        plain = torch.clamp(net(nobs), -1, 1).numpy()
    assert float(np.abs(got - ref).max()) <= S.bound(float(np.abs(plain - ref).max()))


@pytest.mark.parametrize('change', ['use_attention', 'depth', 'embed_size'])
def test_refused_nets(change):
    """a HopeNet with use_attention=False, with depth=2 or with embed_size=64 raises ValueError and changes no state"""
    from hope_amd import agent_glue as G
    from hope_amd import agents as A
    from hope_amd import policy as P
    cfg = P.actor_configs(use_img=False, use_attention=change != 'use_attention')
    if change == 'depth':
        cfg['attention_configs']['depth'] = 2
    if change == 'embed_size':
        cfg['embed_size'] = 64
    net = P.HopeNet(cfg)
    with pytest.raises(ValueError, match='fused policy forward'):
        G.DeviceActor(CPU_ENV, net)
    ag = A.BatchedPPO(device='cpu', use_img=False, actor_cfg=cfg)
    with pytest.raises(ValueError, match='fused policy forward'):
        G.make_actor('device', CPU_ENV, ag)
    assert getattr(ag, 'device_actor', None) is None
    x = S.inputs(3, 3)
    assert ag.policy_mean(_nobs(x)).shape == (3, 2)                                            # today's path still runs


def test_misuse_of_the_host_twin():
    """HOPE_EINVAL with its text for a shape that is not compiled in, an image token that does not go with n_tokens, a null tensor
    and an empty batch; the output keeps its words"""
    import ctypes as C
    from hope_amd import _lib as L
    lib = L.load_library()
    net = S.make_net('actor', 3)
    p, keep = S.host_params(net)
    x = S.inputs(2, 3)
    out = np.full((2, 2), 7.0, np.float32)
    P = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731

    def call(params=p, shape=(3, 2, 1), lidar=x['lidar'], img=None, b=2):
        return lib.hope_policy_forward_host(C.byref(params) if params is not None else None, *shape, P(lidar), P(x['target']), P(x['mask']), P(img), b, P(out))
    bad = L.PolicyParams.from_buffer_copy(p)
    bad.head2_b = None
    for kw in (dict(shape=(2, 2, 1)), dict(shape=(5, 2, 1)), dict(shape=(3, 3, 1)), dict(shape=(3, 0, 1)), dict(shape=(3, 2, 2)), dict(lidar=None),
               dict(img=np.zeros((2, 128), np.float32)), dict(shape=(4, 2, 1)), dict(b=0), dict(params=bad), dict(params=None)):
        assert call(**kw) == -1 and lib.hope_last_error().decode().startswith('hope_policy_forward_host: bad argument'), kw
    assert (out == 7.0).all()
    assert call() == 0 and np.array_equal(S.words(out), S.words(S.twin(net, x)))


def test_sanitizer_driver_of_the_twin_runs_clean(tmp_path):
    """tests/policy_forward_host_sanitize.cpp, a stand-alone program, compiled by the host compiler with -fsanitize=address,undefined"""
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / 'policy_forward_host_sanitize')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
           '-I' + os.path.join(root, 'include'), '-I' + os.path.join(root, 'hope_amd', 'csrc'),
           os.path.join(root, 'tests', 'policy_forward_host_sanitize.cpp'), '-o', exe]
    # the runtime linked into the program where the compiler can (gcc's switch; clang does so by default and may not know it)
    if subprocess.run(cmd + ['-static-libasan'], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'clean' in r.stdout, (r.returncode, r.stdout, r.stderr)
