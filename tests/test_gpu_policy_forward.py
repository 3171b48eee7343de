"""k_policy_pack / k_policy_forward (hope_amd/csrc/hope_policy_kernel.h) on the device: word for word the host twin, ordered by the
stream they are enqueued on, re-packed after an optimiser step, misused, and inside HopeRollout."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_forward_script as S  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_BATCH = 4099
SIZES = (1, 31, 32, 33, 63, 64, 65, 97, 129, 4099)
SENTINEL = np.float32(-77.25)
EINVAL, ESTATE = -1, -5


@pytest.fixture(scope='module')
def envs():
    """one handle per net kind (a handle holds one shape and one set of packed parameters), the net on the device, its host twin's
    parameters"""
    from hope_amd import ParkingBatch
    out = {}
    for kind, t in S.KINDS:
        net = S.make_net(kind, t)
        e = ParkingBatch(64, 32)
        e.enable_policy(*S.shape_of(net), max_batch=MAX_BATCH)
        dnet = S.make_net(kind, t).to(e.device)
        e.policy_load(dnet)
        out[(kind, t)] = (e, net, dnet, S.host_params(net))
    yield out
    for e, *_ in out.values():
        e.close()


def _dev(env, a, offset=0, tail=0, fill=0.0):
    """the float32 array on the device; offset = 1: in a buffer whose base is 4 bytes past the allocation's; tail: that many more
    words behind it (-> the whole buffer as well)"""
    if a is None:
        return None, None
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.full((a.size + offset + tail,), float(fill), dtype=torch.float32, device=env.device)
    v = buf[offset:offset + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 8 == 4 * offset and v.is_contiguous()
    return v, buf


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and np.array_equal(S.words(got), S.words(want)), (what, float(np.abs(got.astype(np.float64) - want).max()))


@pytest.mark.parametrize('kind,t', S.KINDS)
@pytest.mark.parametrize('b', SIZES)
def test_kernel_equals_the_host_twin_word_for_word(envs, kind, t, b):
    """every output word, from 16-byte aligned bases and from bases 4 bytes past the allocation's (inputs and output); `out` is filled
    with a sentinel beforehand and the sentinel words behind its last row survive"""
    env, net, _, hp = envs[(kind, t)]
    x = S.inputs(b, t)
    want = S.twin(net, x, hp)
    od = want.shape[1]
    for offset in (0, 1):
        d = {k: _dev(env, v, offset)[0] for k, v in x.items()}
        out, buf = _dev(env, np.full((b, od), SENTINEL, np.float32), offset, tail=8, fill=float(SENTINEL))
        got = env.policy_forward(d['lidar'], d['target'], d['mask'], d['img_token'], out=out)
        assert got is out
        _same(out, want, (kind, t, b, offset))
        assert not (out.cpu().numpy() == SENTINEL).any()
        whole = buf.cpu().numpy()
        assert (whole[:offset] == SENTINEL).all() and (whole[offset + b * od:] == SENTINEL).all(), 'words outside out were written'
    # the persistent output of this batch size
    d = {k: _dev(env, v)[0] for k, v in x.items()}
    got = env.policy_forward(d['lidar'], d['target'], d['mask'], d['img_token'])
    assert got is env._policy_out[b]
    _same(got, want, (kind, t, b, 'persistent'))


def test_load_and_forward_are_ordered_by_their_stream():
    """torch produces the inputs and the parameters on a side stream, the load and the forward are enqueued there and the result is
    copied back there: nothing synchronises the host in between"""
    from hope_amd import ParkingBatch
    b, t = 4099, 3
    net = S.make_net('actor', t)
    x = S.inputs(b, t, seed=9)
    want = S.twin(net, x)
    e = ParkingBatch(16, 32)
    e.enable_policy(*S.shape_of(net), max_batch=b)
    side = torch.cuda.Stream(device=e.device)
    hx = {k: torch.from_numpy(v.copy()).pin_memory() for k, v in x.items() if v is not None}
    hnet = S.make_net('actor', t)
    for p in hnet.parameters():
        p.data = p.data.pin_memory()
    torch.cuda.synchronize(e.device)
    with torch.cuda.stream(side):
        dnet = S.make_net('actor', t)
        for p, q in zip(dnet.parameters(), hnet.parameters()):
            p.data = (q.data.to(e.device, non_blocking=True) * 2.0) * 0.5
        dx = {k: v.to(e.device, non_blocking=True) for k, v in hx.items()}
        for _ in range(40):                                        # some work in front of the values the calls read
            dx = {k: (v * 2.0) * 0.5 for k, v in dx.items()}
        e.policy_load(dnet)
        got = e.policy_forward(dx['lidar'], dx['target'], dx['mask']).cpu()
    _same(got, want, 'side stream')
    torch.cuda.synchronize(e.device)
    e.close()


def test_repack_after_an_optimiser_step_on_the_device():
    """a forward, an in-place Adam step on the device parameters, another forward: the second equals the twin on the new weights, and a
    third call with nothing changed adds no pack"""
    from hope_amd import ParkingBatch
    from hope_amd import agent_glue as G
    b, t = 65, 3
    e = ParkingBatch(16, 32)
    net = S.make_net('actor', t).to(e.device)
    x = S.inputs(b, t, seed=3)
    nobs = {'lidar': torch.from_numpy(x['lidar']).to(e.device), 'target': torch.from_numpy(x['target']).to(e.device),
            'action_mask': torch.from_numpy(x['mask']).to(e.device)}
    actor = G.DeviceActor(e, net)
    first = actor(nobs).cpu().numpy()
    _same(first, np.clip(S.twin(_cpu(net), x), -1, 1), 'first')
    assert actor.packs == 1
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    for i, p in enumerate(net.parameters()):
        p.grad = torch.sin(torch.arange(p.numel(), device=e.device, dtype=torch.float32) + i).view(p.shape)
    opt.step()
    second = actor(nobs).cpu().numpy()
    assert actor.packs == 2
    _same(second, np.clip(S.twin(_cpu(net), x), -1, 1), 'after the step')
    assert not np.array_equal(S.words(first), S.words(second))
    third = actor(nobs).cpu().numpy()
    assert actor.packs == 2
    _same(third, second, 'unchanged')
    e.close()


def test_two_actors_over_one_env_do_not_share_weights():
    """a handle holds one shape and one set of packed parameters: an actor and a critic net (and a second actor net of the same shape)
    taking turns on one env each give their own twin's words, re-packing when another ran in between and not otherwise"""
    from hope_amd import ParkingBatch
    from hope_amd import agent_glue as G
    b, t = 33, 3
    e = ParkingBatch(16, 32)
    x = S.inputs(b, t, seed=8)
    nobs = {'lidar': torch.from_numpy(x['lidar']).to(e.device), 'target': torch.from_numpy(x['target']).to(e.device),
            'action_mask': torch.from_numpy(x['mask']).to(e.device)}
    nets = [S.make_net('actor', t), S.make_net('critic', t), S.det_fill(S.make_net('actor', t), salt=1.5)]
    want = [np.clip(S.twin(n, x), -1, 1) for n in nets]
    acts = [G.DeviceActor(e, copy_net.to(e.device)) for copy_net in (_cpu(n) for n in nets)]
    for turn in range(2):
        for a, w in zip(acts, want):
            _same(a(nobs), w, ('turn', turn))
            _same(a(nobs), w, ('again', turn))
    assert [a.packs for a in acts] == [2, 2, 2]
    e.close()


def _cpu(net):
    import copy
    return copy.deepcopy(net).cpu()


def test_misuse_fails_loudly():
    """HOPE_ESTATE before the enable and before the first load; HOPE_EINVAL, each with its text, for a shape that is not compiled in, a
    NULL or misaligned parameter tensor, a NULL or misaligned input or output, a batch of 0 and of max_batch + 1, an image token with
    n_tokens 3 and none with n_tokens 4 -- each refused before anything is launched: the packed parameters and the output keep
    their words"""
    from hope_amd import ParkingBatch
    from hope_amd import _lib as L
    mb, t = 40, 3
    e = ParkingBatch(16, 32)
    dev, lib, h = e.device, e.lib, e.h
    net = S.make_net('actor', t)
    dnet = S.make_net('actor', t).to(dev)
    x = S.inputs(mb + 1, t)
    d = {k: torch.from_numpy(v).to(dev) for k, v in x.items() if v is not None}
    out = torch.full((mb + 1, 2), float(SENTINEL), device=dev)
    token = torch.zeros((mb + 1, 128), device=dev)
    P = lambda q: None if q is None else C.c_void_p(q if isinstance(q, int) else q.data_ptr())  # noqa: E731
    err = lambda: lib.hope_last_error().decode()  # noqa: E731
    params, keep = L.policy_params('hope_env_policy_load', dnet, dev)

    def fwd(batch=mb, **ptr):
        a = {'lidar': d['lidar'], 'target': d['target'], 'mask': d['mask'], 'img_token': None, 'out': out}
        a.update(ptr)
        return lib.hope_env_policy_forward(h, *(P(a[k]) for k in ('lidar', 'target', 'mask', 'img_token')), batch, P(a['out']), e._stream())

    assert lib.hope_env_policy_load(h, C.byref(params), None) == ESTATE and 'hope_env_policy_enable first' in err()
    assert fwd() == ESTATE and 'hope_env_policy_enable first' in err()
    for shape in ((2, 2, 1, mb), (5, 2, 1, mb), (3, 0, 1, mb), (3, 3, 1, mb), (3, 2, 2, mb), (3, 2, 1, 0), (3, 2, 1, L.POLICY_MAX_BATCH + 1)):
        assert lib.hope_env_policy_enable(h, *shape) == EINVAL and err().startswith('hope_env_policy_enable:'), shape
    assert fwd() == ESTATE                                         # a refused enable enabled nothing
    with pytest.raises(ValueError):
        e.enable_policy(n_tokens=5)
    e.enable_policy(3, 2, True, max_batch=mb)
    assert fwd() == ESTATE and 'hope_env_policy_load first' in err()
    assert lib.hope_env_policy_load(h, None, None) == EINVAL and 'null parameter struct' in err()
    e.policy_load(dnet)
    want = S.twin(net, {k: (None if v is None else v[:mb]) for k, v in x.items()})
    assert fwd() == 0
    _same(out[:mb], want, 'good call')
    out.fill_(float(SENTINEL))
    # a load that fails leaves the packed parameters as they are
    for field, _ in L.POLICY_FIELDS[::5]:
        bad = L.PolicyParams.from_buffer_copy(params)
        setattr(bad, field, None)
        assert lib.hope_env_policy_load(h, C.byref(bad), None) == EINVAL and 'null tensor' in err(), field
        setattr(bad, field, getattr(params, field) + 2)
        assert lib.hope_env_policy_load(h, C.byref(bad), None) == EINVAL and 'misaligned tensor' in err(), field
    for k in ('lidar', 'target', 'mask', 'out'):
        assert fwd(**{k: None}) == EINVAL and 'null lidar / target / mask / out' in err(), k
        base = out if k == 'out' else d[k]
        assert fwd(**{k: base.data_ptr() + 2}) == EINVAL and 'misaligned buffer' in err(), k
    assert fwd(img_token=token) == EINVAL and 'there is no image token' in err()
    assert fwd(batch=0) == EINVAL and fwd(batch=-1) == EINVAL and fwd(batch=mb + 1) == EINVAL and f'max_batch ({mb})' in err()
    with pytest.raises(L.HopeError, match='lidar must be float32'):
        e.policy_forward(d['lidar'].double(), d['target'], d['mask'])
    with pytest.raises(ValueError, match='enabled for'):
        e.policy_load(S.make_net('critic', t).to(dev))
    torch.cuda.synchronize(dev)
    assert (out.cpu().numpy() == SENTINEL).all(), 'a refused call wrote to out'
    assert fwd() == 0
    _same(out[:mb], want, 'after the refused calls')               # the packed parameters are the loaded ones
    # n_tokens 4: the token is required; another shape drops the parameters; a larger max_batch keeps them
    e.enable_policy(3, 2, True, max_batch=mb + 1)
    assert fwd(batch=mb + 1) == 0
    e.enable_policy(4, 2, True, max_batch=mb)
    assert fwd(img_token=token) == ESTATE and 'hope_env_policy_load first' in err()
    e.policy_load(S.make_net('actor', 4).to(dev))
    assert fwd() == EINVAL and 'the image token is missing' in err()
    assert fwd(img_token=token) == 0
    e.disable_policy()
    assert fwd(img_token=token) == ESTATE
    e.close()


class _TwinActor:
    """stands in as agent.device_actor: the host twin on the same observations"""

    def __init__(self, net):
        self.net, self.means = net, []

    def __call__(self, nobs):
        cpu = _cpu(self.net)
        x = {'lidar': nobs['lidar'].float().cpu().numpy(), 'target': nobs['target'].float().cpu().numpy(),
             'mask': nobs['action_mask'].float().cpu().numpy(), 'img_token': None}
        out = torch.from_numpy(S.twin(cpu, x)).to(nobs['lidar'].device)
        return torch.clamp(out, -1, 1)


def _lots(n, seed=11):
    from hope_amd import ParkingBatch
    from hope_amd.scene_gen import mixed_arrays
    arrs = mixed_arrays(n, levels=('Normal', 'Complex', 'Extrem'), seed=seed, max_obst=32)
    e = ParkingBatch(n, 32)
    e.set_scene_arrays(np.arange(n), *arrs[:5])
    return e


def test_in_the_rollout():
    """HopeRollout(actor='device', chooser='device', obs_norm='device', ring='device', use_planner='device'), 192 scenes, 8 steps,
    against the same rollout on a second handle whose device_actor calls the host twin: actions, log-probabilities, ring contents and
    tallies word for word.  The default path (actor=None) on the same seed: on its own observations the fused forward is within the
    bound of the accuracy test of torch's float64 forward; the share of scene-steps whose chosen action differs from the device run
    is printed, not asserted (a draw next to a threshold may flip)."""
    from hope_amd import agents as A
    from hope_amd import agent_glue as G
    from hope_amd.rollout import HopeRollout
    n, steps, runs = 192, 8, {}
    kw = dict(chooser='device', obs_norm='device', ring='device', use_planner='device')
    worst = [0.0, 0.0]
    for which in ('device', 'twin', 'default'):
        e = _lots(n)
        torch.manual_seed(0)
        ag = A.BatchedPPO(device=e.device, use_img=False)
        ro = HopeRollout(e, ag, steps, seed=4, actor='device' if which == 'device' else None, **kw)
        if which == 'twin':
            ag.device_actor = _TwinActor(ag.actor)
        if which == 'default':
            probe, inner = G.DeviceActor(e, ag.actor), ag.policy_mean

            def policy_mean(nobs, inner=inner, probe=probe, ag=ag):
                mean = inner(nobs)
                ref = torch.clamp(_cpu(ag.actor).double()({k: v.double().cpu() for k, v in nobs.items()}), -1, 1).numpy()
                worst[0] = max(worst[0], float(np.abs(mean.double().cpu().numpy() - ref).max()))
                worst[1] = max(worst[1], float(np.abs(probe(nobs).double().cpu().numpy() - ref).max()))
                return mean
            ag.policy_mean = policy_mean
        for _ in range(steps):
            ro.collect_step()
        r = ro.ring
        runs[which] = ([q.cpu().numpy().copy() for q in (r.action, r.log_prob, r.reward, r.done, r.obs['lidar'], r.obs['target'], r.obs['action_mask'])],
                       ro.stats())
        if which == 'device':
            assert ro.device_actor.on_device and ro.device_actor.packs == 1
        e.close()
    for a, b in zip(runs['device'][0], runs['twin'][0]):
        _same(a, b, 'ring contents')
    assert runs['device'][1] == runs['twin'][1], (runs['device'][1], runs['twin'][1])
    e_torch, e_dev = worst
    print(f'in the loop: e_torch {e_torch:.3e}, e_device {e_dev:.3e}, bound {S.bound(e_torch):.3e}')
    assert e_dev <= S.bound(e_torch), (e_dev, e_torch)
    differs = np.any(runs['device'][0][0] != runs['default'][0][0], axis=-1)
    print(f'scene-steps whose action differs from the default path: {int(differs.sum())} of {differs.size} ({differs.mean():.4f})')
