"""k_imgenc_pack / k_imgenc_conv / k_imgenc_head (hope_amd/csrc/hope_imgenc_kernel.h) on the device: word for word the host twin, on
programmed weights, ordered by the stream they are enqueued on, re-packed after an optimiser step, next to the policy forward on one
handle, misused, on the env's own images and inside HopeRollout."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import img_encoder_script as S  # noqa: E402
import policy_forward_script as PS  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_BATCH = 129
SENTINEL = np.float32(-77.25)
EINVAL, ESTATE = -1, -5
_WANT = {}


def _cpu(net):
    return copy.deepcopy(net).cpu()


def _want(act, b):
    """the twin's (token, features) on images(b, seed=b), once per (act, b)"""
    if (act, b) not in _WANT:
        _WANT[(act, b)] = S.twin(S.make_net(act), S.images(b, seed=b))
    return _WANT[(act, b)]


@pytest.fixture(scope='module')
def envs():
    """one handle per activation, the net on the device"""
    from hope_amd import ParkingBatch
    out = {}
    for act in S.ACTS:
        e = ParkingBatch(64, 32)
        e.enable_img_encoder(act, max_batch=MAX_BATCH)
        dnet = S.make_net(act).to(e.device)
        e.img_encoder_load(dnet)
        out[act] = (e, dnet)
    yield out
    for e, _ in out.values():
        e.close()


def _dev(env, a, offset=0, tail=0, fill=0.0):
    """the array on the device; offset = 1: in a buffer whose base is 4 bytes past the allocation's; tail: that many more elements
    behind it (-> the view and the whole buffer)"""
    a = np.ascontiguousarray(a)
    lead = offset * (4 // a.itemsize)
    buf = torch.full((a.size + lead + tail,), fill, dtype=torch.from_numpy(a[:0].copy()).dtype, device=env.device)
    v = buf[lead:lead + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 8 == 4 * offset and v.is_contiguous()
    return v, buf


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and np.array_equal(S.words(got), S.words(want)), (what, float(np.abs(got.astype(np.float64) - want).max()))


@pytest.mark.parametrize('act', S.ACTS)
@pytest.mark.parametrize('b', S.BATCHES)
def test_kernels_equal_the_host_twin_word_for_word(envs, act, b):
    """token and features, from aligned bases and from bases 4 bytes past the allocation's (image, token and features); both outputs
    are filled with a sentinel beforehand and the sentinel words around them survive; features=False gives the same token"""
    env, _ = envs[act]
    img = S.images(b, seed=b)
    wt, wf = _want(act, b)
    for offset in (0, 1):
        dimg, _ = _dev(env, img, offset)
        token, tbuf = _dev(env, np.full((b, 128), SENTINEL, np.float32), offset, tail=8, fill=float(SENTINEL))
        feat, fbuf = _dev(env, np.full((b, 2048), SENTINEL, np.float32), offset, tail=8, fill=float(SENTINEL))
        got = env.img_encoder_forward(dimg, out=token, features=feat)
        assert got[0] is token and got[1] is feat
        _same(token, wt, (act, b, offset, 'token'))
        _same(feat, wf, (act, b, offset, 'features'))
        for whole, n in ((tbuf.cpu().numpy(), b * 128), (fbuf.cpu().numpy(), b * 2048)):
            assert (whole[:offset] == SENTINEL).all() and (whole[offset + n:] == SENTINEL).all(), 'words outside an output were written'
        token.fill_(float(SENTINEL))
        assert env.img_encoder_forward(dimg, out=token) is token                      # the features stay in the handle
        _same(token, wt, (act, b, offset, 'token alone'))
    # the persistent outputs of this batch size
    dimg, _ = _dev(env, img)
    got = env.img_encoder_forward(dimg)
    assert got is env._imgenc_out[b][0]
    _same(got, wt, (act, b, 'persistent'))
    t2, f2 = env.img_encoder_forward(dimg, features=True)
    assert t2 is got and f2 is env._imgenc_out[b][1]
    _same(f2, wf, (act, b, 'persistent features'))


def test_one_kernel_alone(envs):
    """hope_debug_imgenc_stage (the timing tool's hook): stage 0 writes the features and leaves the token, stage 1 turns them into the
    token; a stage that does not exist or a missing feature buffer is refused and writes nothing"""
    env, _ = envs['tanh']
    b = 33
    wt, wf = _want('tanh', b)
    dimg, _ = _dev(env, S.images(b, seed=b))
    token = torch.full((b, 128), float(SENTINEL), device=env.device)
    feat = torch.full((b, 2048), float(SENTINEL), device=env.device)
    P = lambda q: None if q is None else C.c_void_p(q.data_ptr())  # noqa: E731
    stage = lambda k, f=feat: env.lib.hope_debug_imgenc_stage(env.h, k, P(dimg), b, P(token), P(f), env._stream())  # noqa: E731
    assert stage(2) == EINVAL and stage(-1) == EINVAL and stage(0, None) == EINVAL and stage(1, None) == EINVAL
    assert env.lib.hope_last_error().decode().startswith('hope_debug_imgenc_stage:')
    assert (token.cpu().numpy() == SENTINEL).all() and (feat.cpu().numpy() == SENTINEL).all()
    assert stage(0) == 0
    _same(feat, wf, 'stage 0')
    assert (token.cpu().numpy() == SENTINEL).all()
    assert stage(1) == 0
    _same(token, wt, 'stage 1')


@pytest.mark.parametrize('act', S.ACTS)
def test_orientation_on_the_device(act):
    """the eighteen one-tap weight sets, the shortcut and the fc1-column sets at B = 2 against the twin: programmed weights take no other
    path than dense ones"""
    from hope_amd import ParkingBatch
    e = ParkingBatch(16, 32)
    e.enable_img_encoder(act, max_batch=2)
    img = S.probe_images()[:2]
    dimg = torch.from_numpy(img).to(e.device)
    for name, net in S.orientation_cases(act) + S.shortcut_cases(act) + S.fc1_cases(act):
        wt, wf = S.twin(net, img)
        assert wf.any(), name
        e.img_encoder_load(copy.deepcopy(net).to(e.device))
        token, feat = e.img_encoder_forward(dimg, features=True)
        _same(token, wt, (name, 'token'))
        _same(feat, wf, (name, 'features'))
    e.close()


def test_load_and_forward_are_ordered_by_their_stream():
    """torch produces the images and the parameters on a side stream, the load and the forward are enqueued there and the result is
    copied back there: nothing synchronises the host in between"""
    from hope_amd import ParkingBatch
    b = 129
    wt, wf = _want('tanh', b)
    e = ParkingBatch(16, 32)
    e.enable_img_encoder('tanh', max_batch=b)
    side = torch.cuda.Stream(device=e.device)
    himg = torch.from_numpy(S.images(b, seed=b)).pin_memory()
    hnet = S.make_net('tanh')
    for p in hnet.parameters():
        p.data = p.data.pin_memory()
    torch.cuda.synchronize(e.device)
    with torch.cuda.stream(side):
        dnet = S.make_net('tanh')
        for p, q in zip(dnet.parameters(), hnet.parameters()):
            p.data = (q.data.to(e.device, non_blocking=True) * 2.0) * 0.5
        dimg = himg.to(e.device, non_blocking=True)
        for _ in range(40):                                        # some work in front of the values the calls read
            dimg = (dimg ^ 255) ^ 255
        e.img_encoder_load(dnet)
        token, feat = e.img_encoder_forward(dimg, features=True)
        token, feat = token.cpu(), feat.cpu()
    _same(token, wt, 'side stream token')
    _same(feat, wf, 'side stream features')
    torch.cuda.synchronize(e.device)
    e.close()


def test_repack_after_an_optimiser_step_on_the_device():
    """a forward, an in-place Adam step on the device parameters, another forward: the second equals the twin on the new weights, and a
    third call with nothing changed adds no pack"""
    from hope_amd import ParkingBatch
    from hope_amd import agent_glue as G
    b = 33
    e = ParkingBatch(16, 32)
    net = S.make_net('tanh').to(e.device)
    img = S.images(b, seed=6)
    dimg = torch.from_numpy(img).to(e.device)
    enc = G.DeviceImgEncoder(e, net)
    assert enc.on_device
    first = enc(dimg).cpu().numpy()
    _same(first, S.twin(_cpu(net), img)[0], 'first')
    assert enc.packs == 1
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    for i, p in enumerate(net.parameters()):
        p.grad = torch.sin(torch.arange(p.numel(), device=e.device, dtype=torch.float32) + i).view(p.shape)
    opt.step()
    second = enc(dimg).cpu().numpy()
    assert enc.packs == 2
    _same(second, S.twin(_cpu(net), img)[0], 'after the step')
    assert not np.array_equal(S.words(first), S.words(second))
    third = enc(dimg).cpu().numpy()
    assert enc.packs == 2
    _same(third, second, 'unchanged')
    e.close()


def test_sharing_a_handle():
    """two encoders (tanh and leaky nets) take turns on one env, each re-packing when the other ran in between and not otherwise; the
    encoder and the policy coexist: enable_policy after enable_img_encoder and the reverse leave the other's packed words and outputs
    as they were, and DeviceActor(img_encoder='device') equals the twins' composition"""
    from hope_amd import ParkingBatch
    from hope_amd import agent_glue as G
    b = 33
    e = ParkingBatch(16, 32)
    img = S.images(b, seed=8)
    dimg = torch.from_numpy(img).to(e.device)
    nets = [S.make_net('tanh'), S.make_net('leaky'), S.det_fill(S.make_net('tanh'), salt=1.5)]
    want = [S.twin(n, img)[0] for n in nets]
    encs = [G.DeviceImgEncoder(e, _cpu(n).to(e.device)) for n in nets]
    for turn in range(2):
        for enc, w in zip(encs, want):
            _same(enc(dimg), w, ('turn', turn))
            _same(enc(dimg), w, ('again', turn))
    assert [enc.packs for enc in encs] == [2, 2, 2]
    # the policy is enabled AFTER the encoder: the encoder's packed words and its output stay
    x = PS.inputs(b, 4, seed=2)
    dx = {k: torch.from_numpy(v).to(e.device) for k, v in x.items()}
    pnet = nets[2]
    e.enable_policy(*PS.shape_of(pnet), max_batch=b)
    e.policy_load(_cpu(pnet).to(e.device))
    pwant = PS.twin(pnet, x)
    _same(e.policy_forward(dx['lidar'], dx['target'], dx['mask'], dx['img_token']), pwant, 'policy next to the encoder')
    _same(e.img_encoder_forward(dimg), want[2], 'encoder after enable_policy')            # no load in between: the packed words are the last encoder's
    # the encoder is enabled again (more room) and disabled and enabled AFTER the policy: the policy's packed words and output stay
    e.enable_img_encoder('tanh', max_batch=2 * b)
    _same(e.img_encoder_forward(dimg), want[2], 'encoder after more room')
    e.disable_img_encoder()
    _same(e.policy_forward(dx['lidar'], dx['target'], dx['mask'], dx['img_token']), pwant, 'policy after disable_img_encoder')
    e.enable_img_encoder('tanh', max_batch=b)
    e.img_encoder_load(_cpu(nets[0]).to(e.device))
    _same(e.img_encoder_forward(dimg), want[0], 'encoder enabled after the policy')
    _same(e.policy_forward(dx['lidar'], dx['target'], dx['mask'], dx['img_token']), pwant, 'policy after the encoder')
    # the actor with its encoder on the device: the twins' composition
    dnet = _cpu(nets[0]).to(e.device)
    actor = G.DeviceActor(e, dnet, img_encoder='device')
    nobs = {'lidar': dx['lidar'], 'target': dx['target'], 'action_mask': dx['mask'], 'img': dimg}
    _same(actor(nobs), np.clip(PS.twin(nets[0], dict(x, img_token=want[0])), -1, 1), 'actor with the device encoder')
    assert actor.packs == 1 and actor.img_encoder.packs == 1
    e.close()


def test_misuse_fails_loudly():
    """HOPE_ESTATE before the enable and before the first load; HOPE_EINVAL, each with its text, for an act that is not compiled in, a
    max_batch out of range, a NULL or misaligned parameter tensor, a NULL or misaligned image, token or feature buffer, a batch of 0 and
    of max_batch + 1 -- each refused before anything is launched: the packed parameters and the outputs keep their words"""
    from hope_amd import ParkingBatch
    from hope_amd import _lib as L
    mb = 5
    e = ParkingBatch(16, 32)
    dev, lib, h = e.device, e.lib, e.h
    net = S.make_net('tanh')
    dnet = S.make_net('tanh').to(dev)
    img = S.images(mb + 1, seed=3)
    dimg = torch.from_numpy(img).to(dev)
    token = torch.full((mb + 1, 128), float(SENTINEL), device=dev)
    feat = torch.full((mb + 1, 2048), float(SENTINEL), device=dev)
    P = lambda q: None if q is None else C.c_void_p(q if isinstance(q, int) else q.data_ptr())  # noqa: E731
    err = lambda: lib.hope_last_error().decode()  # noqa: E731
    params, keep = L.imgenc_params('hope_env_imgenc_load', dnet, dev)

    def fwd(batch=mb, **ptr):
        a = {'img': dimg, 'token': token, 'feat': feat}
        a.update(ptr)
        return lib.hope_env_imgenc_forward(h, P(a['img']), batch, P(a['token']), P(a['feat']), e._stream())

    assert lib.hope_env_imgenc_load(h, C.byref(params), None) == ESTATE and 'hope_env_imgenc_enable first' in err()
    assert fwd() == ESTATE and 'hope_env_imgenc_enable first' in err()
    for act, room in ((2, mb), (-1, mb), (0, 0), (0, L.IMGENC_MAX_BATCH + 1)):
        assert lib.hope_env_imgenc_enable(h, act, room) == EINVAL and err().startswith('hope_env_imgenc_enable:'), (act, room)
    assert fwd() == ESTATE                                         # a refused enable enabled nothing
    with pytest.raises(ValueError, match="'tanh' or 'leaky'"):
        e.enable_img_encoder('relu')
    with pytest.raises(L.HopeError, match='enable_img_encoder first'):
        e.img_encoder_load(dnet)
    e.enable_img_encoder('tanh', max_batch=mb)
    assert fwd() == ESTATE and 'hope_env_imgenc_load first' in err()
    assert lib.hope_env_imgenc_load(h, None, None) == EINVAL and 'null parameter struct' in err()
    e.img_encoder_load(dnet)
    wt, wf = S.twin(net, img[:mb])
    assert fwd() == 0
    _same(token[:mb], wt, 'good call')
    _same(feat[:mb], wf, 'good call, features')
    token.fill_(float(SENTINEL))
    feat.fill_(float(SENTINEL))
    # a load that fails leaves the packed parameters as they are
    for field, _, _ in L.IMGENC_FIELDS[::3]:
        bad = L.ImgEncParams.from_buffer_copy(params)
        setattr(bad, field, None)
        assert lib.hope_env_imgenc_load(h, C.byref(bad), None) == EINVAL and 'null tensor' in err(), field
        setattr(bad, field, getattr(params, field) + 2)
        assert lib.hope_env_imgenc_load(h, C.byref(bad), None) == EINVAL and 'misaligned tensor' in err(), field
    for k in ('img', 'token'):
        assert fwd(**{k: None}) == EINVAL and 'null img / token' in err(), k
    for k, base in (('img', dimg), ('token', token), ('feat', feat)):
        for off in (1, 2) if k == 'img' else (2,):
            assert fwd(**{k: base.data_ptr() + off}) == EINVAL and 'misaligned buffer' in err(), (k, off)
    assert fwd(batch=0) == EINVAL and fwd(batch=-1) == EINVAL and fwd(batch=mb + 1) == EINVAL and f'max_batch ({mb})' in err()
    with pytest.raises(L.HopeError, match='img must be uint8'):
        e.img_encoder_forward(dimg.float())
    with pytest.raises(ValueError, match='enabled for'):
        e.img_encoder_load(S.make_net('leaky').to(dev))
    torch.cuda.synchronize(dev)
    assert (token.cpu().numpy() == SENTINEL).all() and (feat.cpu().numpy() == SENTINEL).all(), 'a refused call wrote to an output'
    assert fwd(feat=None) == 0
    _same(token[:mb], wt, 'after the refused calls')               # the packed parameters are the loaded ones
    assert (feat.cpu().numpy() == SENTINEL).all()
    e.enable_img_encoder('tanh', max_batch=mb + 1)                 # more room keeps the parameters
    assert fwd(batch=mb + 1) == 0
    e.disable_img_encoder()
    assert fwd() == ESTATE
    e.close()


def test_a_batch_whose_bytes_pass_two_to_the_31():
    """B = 174 800 images are 2.15e9 bytes: the last rows, the row at the 2^31 boundary and row 0 equal the twin on the downloaded
    bytes (the kernels index with 64 bits), and row i equals the same image in a batch of its own"""
    from hope_amd import ParkingBatch
    b = 174800
    e = ParkingBatch(16, 32)
    net = S.make_net('tanh')
    e.enable_img_encoder('tanh', max_batch=b)
    e.img_encoder_load(_cpu(net).to(e.device))
    g = torch.Generator(device=e.device).manual_seed(5)
    img = torch.randint(0, 256, (b, 3, 64, 64), dtype=torch.uint8, device=e.device, generator=g)
    token = e.img_encoder_forward(img)
    rows = [0, 2 ** 31 // 12288 - 1, 2 ** 31 // 12288, 2 ** 31 // 12288 + 1, b - 2, b - 1]
    at = torch.tensor(rows, device=e.device)
    got = token[at].cpu().numpy()
    _same(got, S.twin(net, img[at].cpu().numpy())[0], 'rows around 2^31 bytes')
    _same(e.img_encoder_forward(img[b - 33:].contiguous()), token[b - 33:].cpu().numpy(), 'the last tile on its own')
    e.close()


def _lots(n, seed=11, image=True):
    from hope_amd import ParkingBatch
    from hope_amd.scene_gen import mixed_arrays
    arrs = mixed_arrays(n, levels=('Normal', 'Complex', 'Extrem'), seed=seed, max_obst=32)
    e = ParkingBatch(n, 32, image=image)
    e.set_scene_arrays(np.arange(n), *arrs[:5])
    return e


def test_on_the_envs_own_images():
    """192 lots with the image flag, 4 steps with HOPE_STAGE_IMG: at every step the kernels' token on the env's own `img` tensor (no
    copy) equals the twin's on the downloaded bytes"""
    n = 192
    e = _lots(n)
    net = S.make_net('tanh')
    e.enable_img_encoder('tanh')
    e.img_encoder_load(_cpu(net).to(e.device))
    hp = S.host_params(net)
    rng = np.random.default_rng(5)
    e.reset_obs()
    seen = set()
    for step in range(5):
        assert e.img.dtype == torch.uint8 and tuple(e.img.shape) == (n, 3, 64, 64)
        token = e.img_encoder_forward(e.img)
        host = e.img.cpu().numpy()
        assert host.any() and len(np.unique(host)) > 2
        _same(token, S.twin(net, host, hp)[0], ('step', step))
        seen.add(host.tobytes())
        if step < 4:
            e.step(torch.from_numpy(rng.uniform(-1, 1, (n, 2))).to(e.device, e.action_dtype))
    assert len(seen) == 5                                          # the images moved
    e.close()


class _TwinActor:
    """stands in as agent.device_actor: the host twins of the encoder and of the forward on the same observations"""

    def __init__(self, net):
        self.net = net

    def __call__(self, nobs):
        cpu = _cpu(self.net)
        token, _ = S.twin(cpu, nobs['img'].cpu().numpy())
        x = {'lidar': nobs['lidar'].float().cpu().numpy(), 'target': nobs['target'].float().cpu().numpy(),
             'mask': nobs['action_mask'].float().cpu().numpy(), 'img_token': token}
        return torch.clamp(torch.from_numpy(PS.twin(cpu, x)).to(nobs['lidar'].device), -1, 1)


def test_in_the_rollout():
    """HopeRollout with a use_img PPO agent, actor='device', img_encoder='device', 192 lots, 4 steps, against the same rollout whose
    device_actor calls the two host twins: actions and ring contents word for word.  The default torch path on the same seed: on its
    own observations the device actor's output is within policy_forward_script.bound of torch's float64 forward."""
    from hope_amd import agents as A
    from hope_amd import agent_glue as G
    from hope_amd.rollout import HopeRollout
    n, steps, runs = 192, 4, {}
    kw = dict(chooser='device', obs_norm='device', ring='device', use_planner='device')
    worst = [0.0, 0.0]
    for which in ('device', 'twin', 'default'):
        e = _lots(n)
        torch.manual_seed(0)
        ag = A.BatchedPPO(device=e.device, use_img=True)
        ro = HopeRollout(e, ag, steps, seed=4, actor='device' if which == 'device' else None, img_encoder='device' if which == 'device' else None, **kw)
        if which == 'twin':
            ag.device_actor = _TwinActor(ag.actor)
        if which == 'default':
            probe, inner = G.DeviceActor(e, ag.actor, img_encoder='device'), ag.policy_mean

            def policy_mean(nobs, inner=inner, probe=probe, ag=ag):
                mean = inner(nobs)
                ref = torch.clamp(_cpu(ag.actor).double()({k: (v.cpu() if v.dtype == torch.uint8 else v.double().cpu()) for k, v in nobs.items()}), -1, 1)
                ref = ref.detach().numpy()
                worst[0] = max(worst[0], float(np.abs(mean.double().cpu().numpy() - ref).max()))
                worst[1] = max(worst[1], float(np.abs(probe(nobs).double().cpu().numpy() - ref).max()))
                return mean
            ag.policy_mean = policy_mean
        for _ in range(steps):
            ro.collect_step()
        r = ro.ring
        runs[which] = [q.cpu().numpy().copy() for q in (r.action, r.log_prob, r.reward, r.done, r.obs['lidar'], r.obs['target'], r.obs['action_mask'])]
        runs[which].append(r.obs['img'].cpu().numpy().copy())
        if which == 'device':
            da = ro.device_actor
            assert da.on_device and da.packs == 1 and da.img_encoder.on_device and da.img_encoder.packs == 1
        e.close()
    for a, b in zip(runs['device'][:-1], runs['twin'][:-1]):
        _same(a, b, 'ring contents')
    assert np.array_equal(runs['device'][-1], runs['twin'][-1]) and runs['device'][-1].any()
    e_torch, e_dev = worst
    print(f'in the loop: e_torch {e_torch:.3e}, e_device {e_dev:.3e}, bound {PS.bound(e_torch):.3e}')
    assert e_dev <= PS.bound(e_torch), (e_dev, e_torch)
