"""The fused image encoder's rule (hope_amd/csrc/hope_imgenc_core.h) through its host twin hope_imgenc_forward_host, on the CPU: its
accuracy against torch's float64 forward next to that of torch's own float32 forward, the orientation of every 3x3 tap, of the 1x1
shortcuts and of fc1's columns, the independence of an image from its batch, agent_glue.DeviceImgEncoder and
DeviceActor(img_encoder='device') on a CPU env, the configurations and calls that are refused, and the sanitizer driver of the twin."""
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
import img_encoder_script as S  # noqa: E402
import policy_forward_script as PS  # noqa: E402

CPU_ENV = types.SimpleNamespace(n=1, device=torch.device('cpu'))


@pytest.mark.parametrize('act', S.ACTS)
def test_accuracy_against_torch_float64(act):
    """features and token at B = 65: e_twin <= 4 max(e_torch, 2^-22 max(1, max|ref|)), both measured against the same module in
    float64 (DESIGN 5n records them).  Measured (e_torch / e_twin): tanh features 4.76e-07 / 5.41e-07, token 4.82e-07 / 4.54e-07;
    leaky features 1.10e-06 / 7.33e-07, token 4.16e-07 / 8.24e-07."""
    net, img, (t64, f64), (t32, f32) = S.reference(act, 65)
    assert not img[0].any() and (img[1] == 255).all() and all(img[2, :, y, x].all() for y, x in ((0, 0), (0, 63), (63, 0), (63, 63)))
    for block, winners in enumerate(S.pool_winners(net, img)):
        assert winners == {(0, 0), (0, 1), (1, 0), (1, 1)}, (block, winners)
    token, feat = S.twin(net, img)
    for name, got, ref, plain in (('features', feat, f64, f32), ('token', token, t64, t32)):
        e_torch, e_twin = S.err(plain, ref), S.err(got, ref)
        print(f'{act} {name}: e_torch {e_torch:.3e}, e_twin {e_twin:.3e}, bound {S.bound(e_torch, ref):.3e}, max|ref| {np.abs(ref).max():.3f}')
        assert np.isfinite(got).all() and e_twin <= S.bound(e_torch, ref), (name, e_twin, e_torch)
        assert float(np.abs(got).max()) > 1e-3 and float(got.std()) > 1e-4                         # not a trivial output


def _nobs(x, img):
    return {'lidar': torch.from_numpy(x['lidar']), 'target': torch.from_numpy(x['target']), 'action_mask': torch.from_numpy(x['mask']),
            'img': torch.from_numpy(img)}


def test_accuracy_of_the_whole_actor():
    """DeviceActor(img_encoder='device') on a CPU env against the module in float64, under policy_forward_script.bound"""
    from hope_amd import agent_glue as G
    net, img = S.make_net('tanh'), S.images(65, seed=2)
    nobs = _nobs(PS.inputs(65, 3, seed=9), img)
    got = G.DeviceActor(CPU_ENV, net, img_encoder='device')(nobs).numpy()
    with torch.no_grad():
        ref = torch.clamp(copy.deepcopy(net).double()({k: (v if v.dtype == torch.uint8 else v.double()) for k, v in nobs.items()}), -1, 1).numpy()
        plain = torch.clamp(net(nobs), -1, 1).numpy()
    e_torch, e_dev = float(np.abs(plain - ref).max()), float(np.abs(got - ref).max())
    print(f'actor with the image encoder: e_torch {e_torch:.3e}, e_device {e_dev:.3e}, bound {PS.bound(e_torch):.3e}')
    assert e_dev <= PS.bound(e_torch), (e_dev, e_torch)


def _nonzero(a):
    return set(np.flatnonzero(a).tolist())


@pytest.mark.parametrize('act', S.ACTS)
def test_orientation_of_every_tap(act):
    """one nonzero 3x3 tap (nine per block), then one nonzero 1x1 weight: the features equal torch's float32 features within the
    bound and are nonzero at exactly torch's indices, on four images of one bright pixel each"""
    img = S.probe_images()
    seen = set()
    for n, (name, net) in enumerate(S.orientation_cases(act) + S.shortcut_cases(act)):
        _, feat = S.twin(net, img)
        _, f32 = S.torch_forward(net, img, torch.float32)
        assert f32.any(), name
        assert S.err(feat, f32.astype(np.float64)) <= S.FACTOR * S.FLOOR * max(1.0, float(np.abs(f32).max())), name
        for i in range(len(img)):
            assert _nonzero(feat[i]) == _nonzero(f32[i].reshape(-1)), (name, i)
        if n < 18:
            seen.add(tuple(sorted(_nonzero(feat))))
    assert len(seen) == 18                                                          # no two taps light the same features


@pytest.mark.parametrize('act', S.ACTS)
def test_orientation_of_fc1_columns(act):
    """fc1 with one nonzero column k in {0, 255, 256, 2047}: the token equals torch's within the bound and differs between the columns"""
    img = S.images(6, seed=4)
    tokens = []
    for name, net in S.fc1_cases(act):
        token, _ = S.twin(net, img)
        (t64, _), (t32, _) = S.torch_forward(net, img, torch.float64), S.torch_forward(net, img, torch.float32)
        assert S.err(token, t64) <= S.bound(S.err(t32, t64), t64), name
        tokens.append(token)
    for i in range(len(tokens)):
        for j in range(i):
            assert float(np.abs(tokens[i] - tokens[j]).max()) > 1e-3, (i, j)


@pytest.mark.parametrize('act', S.ACTS)
def test_an_image_does_not_depend_on_its_batch(act):
    """row i of a B = 67 call equals, word for word, the B = 1 call on image i and the same row after the batch is reversed"""
    net = S.make_net(act)
    hp = S.host_params(net)
    img = S.images(67, seed=1)
    token, feat = S.twin(net, img, hp)
    rt, rf = S.twin(net, img[::-1], hp)
    assert np.array_equal(S.words(rt[::-1]), S.words(token)) and np.array_equal(S.words(rf[::-1]), S.words(feat))
    for i in (0, 1, 31, 32, 33, 63, 64, 65, 66):
        t1, f1 = S.twin(net, img[i:i + 1], hp)
        assert np.array_equal(S.words(t1[0]), S.words(token[i])) and np.array_equal(S.words(f1[0]), S.words(feat[i])), i


def test_device_img_encoder_on_a_cpu_env():
    """one pack on first use, none on the second call; a re-pack after an in-place Adam step that touches an encoder weight and after
    a load_state_dict, each result word-equal to a fresh twin call; a float image goes through torch"""
    from hope_amd import agent_glue as G
    net = S.make_net('tanh')
    img = S.images(9, seed=3)
    timg = torch.from_numpy(img)
    enc = G.DeviceImgEncoder(CPU_ENV, net)
    assert not enc.on_device and enc.packs == 0
    got = enc(timg).numpy()
    assert enc.packs == 1 and np.array_equal(S.words(got), S.words(S.twin(net, img)[0]))
    again, feat = enc(timg, features=True)
    assert enc.packs == 1 and np.array_equal(S.words(again.numpy()), S.words(got)) and np.array_equal(S.words(feat.numpy()), S.words(S.twin(net, img)[1]))
    # an in-place optimiser step on the encoder's weights only
    opt = torch.optim.Adam([net.embed_img.net[0].layer[0].weight, net.embed_img.net[3].weight], lr=1e-3)
    net.re_embed_img(net.embed_img(timg.float() * (1.0 / 255.0))).square().sum().backward()
    opt.step()
    stepped = enc(timg).numpy()
    assert enc.packs == 2 and not np.array_equal(S.words(stepped), S.words(got))
    assert np.array_equal(S.words(stepped), S.words(S.twin(net, img)[0]))
    # a change of a tensor that is not the encoder's does not re-pack
    with torch.no_grad():
        net.embed_lidar[0].weight.mul_(1.5)
    assert np.array_equal(S.words(enc(timg).numpy()), S.words(stepped)) and enc.packs == 2
    net.load_state_dict(S.make_net('tanh').state_dict())
    loaded = enc(timg).numpy()
    assert enc.packs == 3 and np.array_equal(S.words(loaded), S.words(got))
    # a float image: torch, as today
    fimg = timg.float() * (1.0 / 255.0)
    with torch.no_grad():
        want = net.re_embed_img(net.embed_img(fimg))
    assert torch.equal(enc(fimg), want) and enc.packs == 3


def test_device_actor_with_the_device_img_encoder():
    """img_encoder='device' on a CPU env: the twin's token goes into the twin's forward; img_encoder=None gives today's words"""
    from hope_amd import agent_glue as G
    from hope_amd import agents as A
    net = S.make_net('tanh')
    img = S.images(9, seed=5)
    x = PS.inputs(9, 3, seed=2)
    nobs = _nobs(x, img)
    actor = G.DeviceActor(CPU_ENV, net, img_encoder='device')
    got = actor(nobs).numpy()
    assert actor.packs == 1 and actor.img_encoder.packs == 1
    token, _ = S.twin(net, img)
    want = np.clip(PS.twin(net, dict(x, img_token=token)), -1, 1)
    assert np.array_equal(S.words(got), S.words(want))
    assert np.array_equal(S.words(actor(nobs).numpy()), S.words(got)) and actor.packs == 1 and actor.img_encoder.packs == 1
    # a float image: the torch encoder, then the twin's forward
    fobs = dict(nobs, img=nobs['img'].float() * (1.0 / 255.0))
    with torch.no_grad():
        ftoken = net.re_embed_img(net.embed_img(fobs['img'])).numpy()
    assert np.array_equal(S.words(actor(fobs).numpy()), S.words(np.clip(PS.twin(net, dict(x, img_token=ftoken)), -1, 1)))
    # None: exactly what the actor did before the argument existed
    plain = G.DeviceActor(CPU_ENV, net)
    assert plain.img_encoder is None
    with torch.no_grad():
        ttoken = net.re_embed_img(net.embed_img(nobs['img'].to(torch.float32) * (1.0 / 255.0))).numpy()
    assert np.array_equal(S.words(plain(nobs).numpy()), S.words(np.clip(PS.twin(net, dict(x, img_token=ttoken)), -1, 1)))
    # through make_actor and an agent
    torch.manual_seed(0)
    ag = A.BatchedPPO(device='cpu', use_img=True)
    da = G.make_actor('device', CPU_ENV, ag, img_encoder='device')
    assert da is ag.device_actor and da.img_encoder is not None
    assert ag.policy_mean(nobs).shape == (9, 2) and da.img_encoder.packs == 1


@pytest.mark.parametrize('change', ['img_shape', 'img_conv_layers', 'k_img_conv', 'img_linear_layers', 'embed_size', 'use_tanh_activate', 'amp'])
def test_refused_configurations(change):
    """every unsupported configuration raises ValueError('... fused image encoder ...') and leaves the agent usable"""
    from hope_amd import agent_glue as G
    from hope_amd import agents as A
    from hope_amd import policy as P
    cfg = P.actor_configs(use_img=True)
    other = {'img_shape': (3, 32, 32), 'img_conv_layers': [4, 4], 'k_img_conv': 5, 'img_linear_layers': [128], 'embed_size': 64,
             'use_tanh_activate': False}
    if change in other:
        cfg[change] = other[change]
    net = P.HopeNet(cfg)
    if change == 'amp':
        P.set_img_amp(net, True)
    with pytest.raises(ValueError, match='fused image encoder'):
        G.DeviceImgEncoder(CPU_ENV, net)
    with pytest.raises(ValueError, match='fused image encoder'):
        from hope_amd import _lib as L
        L.imgenc_shape(net)
    side = cfg['img_shape'][1]
    x = PS.inputs(3, 3)
    nobs = _nobs(x, np.zeros((3, 3, side, side), np.uint8))
    with torch.no_grad():
        assert net(nobs).shape == (3, 2)                                                          # the net still runs
    if change not in ('embed_size', 'use_tanh_activate', 'amp'):                                  # (these the policy forward refuses too, or are set on the module)
        ag = A.BatchedPPO(device='cpu', use_img=True, actor_cfg=cfg)
        with pytest.raises(ValueError, match='fused image encoder'):
            G.make_actor('device', CPU_ENV, ag, img_encoder='device')
        assert getattr(ag, 'device_actor', None) is None
        assert ag.policy_mean(nobs).shape == (3, 2)                                               # today's path still runs


def test_refused_arguments():
    """img_encoder='device' without actor='device' or without use_img, and a value that is neither None nor 'device'"""
    from hope_amd import agent_glue as G
    from hope_amd import agents as A
    from hope_amd import policy as P
    with_img, without = A.BatchedPPO(device='cpu', use_img=True), A.BatchedPPO(device='cpu', use_img=False)
    with pytest.raises(ValueError, match="needs actor='device'"):
        G.make_actor(None, CPU_ENV, with_img, img_encoder='device')
    with pytest.raises(ValueError, match='use_img'):
        G.make_actor('device', CPU_ENV, without, img_encoder='device')
    with pytest.raises(ValueError, match='use_img'):
        G.DeviceActor(CPU_ENV, P.HopeNet(P.actor_configs(use_img=False)), img_encoder='device')
    with pytest.raises(ValueError, match="None or 'device'"):
        G.make_actor('device', CPU_ENV, with_img, img_encoder='gpu')
    with pytest.raises(ValueError, match='fused image encoder'):
        G.DeviceImgEncoder(CPU_ENV, P.HopeNet(P.actor_configs(use_img=False)))
    for ag in (with_img, without):
        assert getattr(ag, 'device_actor', None) is None


def test_misuse_of_the_host_twin():
    """HOPE_EINVAL with its text for act = 2, a null tensor, batch = 0, a null img and an img off by one byte; the outputs keep
    their sentinel"""
    from hope_amd import _lib as L
    lib = L.load_library()
    net = S.make_net('tanh')
    p, keep = S.host_params(net)
    store = np.zeros(2 * 3 * 64 * 64 + 4, np.uint8)
    img = store[:2 * 3 * 64 * 64]
    token, feat = np.full((2, 128), 7.0, np.float32), np.full((2, 2048), 7.0, np.float32)
    assert img.ctypes.data % 4 == 0
    P = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731

    def call(params=p, act=0, im=img, b=2):
        return lib.hope_imgenc_forward_host(C.byref(params) if params is not None else None, act, P(im), b, P(token), P(feat))
    bad = L.ImgEncParams.from_buffer_copy(p)
    bad.mean_w = None
    for kw in (dict(act=2), dict(act=-1), dict(params=bad), dict(params=None), dict(b=0), dict(im=None), dict(im=store[1:1 + 2 * 3 * 64 * 64])):
        assert call(**kw) == -1 and lib.hope_last_error().decode().startswith('hope_imgenc_forward_host: bad argument'), kw
    assert (token == 7.0).all() and (feat == 7.0).all()
    assert call() == 0
    t, f = S.twin(net, img.reshape(2, 3, 64, 64))
    assert np.array_equal(S.words(token), S.words(t)) and np.array_equal(S.words(feat), S.words(f))


def test_sanitizer_driver_of_the_twin_runs_clean(tmp_path):
    """tests/img_encoder_host_sanitize.cpp, a stand-alone program, compiled by the host compiler with -fsanitize=address,undefined"""
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / 'img_encoder_host_sanitize')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
           '-I' + os.path.join(root, 'include'), '-I' + os.path.join(root, 'hope_amd', 'csrc'),
           os.path.join(root, 'tests', 'img_encoder_host_sanitize.cpp'), '-o', exe]
    # the runtime linked into the program where the compiler can (gcc's switch; clang does so by default and may not know it)
    if subprocess.run(cmd + ['-static-libasan'], capture_output=True).returncode != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'clean' in r.stdout, (r.returncode, r.stdout, r.stderr)
