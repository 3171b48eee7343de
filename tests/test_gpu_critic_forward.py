"""k_critic_pack / k_critic_forward (hope_amd/csrc/hope_critic_kernel.h) on the device: word for word the host twin for every shape,
the parameter slots, DeviceCritics' per-slot re-pack, the order of the stream the calls are enqueued on, misuse, the policy forward
next to it on one handle, and one SAC and one PPO update with the critics on the device."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import critic_forward_script as S  # noqa: E402
import policy_forward_script as PS  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_BATCH = 129
SIZES = (1, 31, 32, 33, 65, 129)
SALTS = (0.3, 0.5, 0.7, 0.9)
SENTINEL = np.float32(-77.25)
EINVAL, ESTATE = -1, -5


@pytest.fixture(scope='module')
def envs():
    """one handle per kind with four slots, nets of four salts loaded into them, and their host twins' parameters"""
    from hope_amd import ParkingBatch
    out = {}
    for kind, t in S.KINDS:
        e = ParkingBatch(16, 32)
        e.enable_critics(4, *S.flags(kind, t), max_batch=MAX_BATCH)
        nets = [S.make_net(kind, t, salt) for salt in SALTS]
        dnets = [copy.deepcopy(n).to(e.device) for n in nets]
        for s, d in enumerate(dnets):
            e.critic_load(s, d)
        out[(kind, t)] = (e, nets, dnets, [S.host_params(n) for n in nets])
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


def _cpu(net):
    return copy.deepcopy(net).cpu()


@pytest.mark.parametrize('kind,t', S.KINDS)
@pytest.mark.parametrize('b', SIZES)
def test_kernel_equals_the_host_twin_word_for_word(envs, kind, t, b):
    """every output word of one net, from 16-byte aligned bases and from bases 4 bytes past the allocation's (inputs and output); `out`
    is filled with a sentinel beforehand and the sentinel words around it survive"""
    env, nets, _, hps = envs[(kind, t)]
    x = S.inputs(b, kind, t)
    want = S.twin(nets[0], x, hps[0])[None]
    for offset in (0, 1):
        d = {k: _dev(env, v, offset)[0] for k, v in x.items()}
        out, buf = _dev(env, np.full((1, b), SENTINEL, np.float32), offset, tail=8, fill=float(SENTINEL))
        got = env.critic_forward((0,), d['lidar'], d['target'], d['mask'], d['img_token'], d['action'], out=out)
        assert got is out
        _same(out, want, (kind, t, b, offset))
        assert not (out.cpu().numpy() == SENTINEL).any()
        whole = buf.cpu().numpy()
        assert (whole[:offset] == SENTINEL).all() and (whole[offset + b:] == SENTINEL).all(), 'words outside out were written'
    d = {k: _dev(env, v)[0] for k, v in x.items()}
    got = env.critic_forward((0,), d['lidar'], d['target'], d['mask'], d['img_token'], d['action'])
    assert got is env._critic_out[(1, b)]
    _same(got, want, (kind, t, b, 'persistent'))


@pytest.mark.parametrize('kind,t', S.KINDS)
def test_slots(envs, kind, t):
    """out[i] is the twin of net slots[i] on its own image token, for one to four slots in any order; reloading slot 1 changes slot 1
    only"""
    env, nets, dnets, hps = envs[(kind, t)]
    b = 33
    x = S.inputs(b, kind, t, seed=3, n_nets=4)
    want = [S.twin(nets[s], x, hps[s], which=s) for s in range(4)]
    assert len({w.tobytes() for w in want}) == 4
    d = {k: _dev(env, v)[0] for k, v in x.items()}

    def run(slots):
        tok = None if d['img_token'] is None else d['img_token'][list(slots)].contiguous()
        out, buf = _dev(env, np.full((len(slots), b), SENTINEL, np.float32), tail=8, fill=float(SENTINEL))
        env.critic_forward(slots, d['lidar'], d['target'], d['mask'], tok, d['action'], out=out)
        assert (buf.cpu().numpy()[len(slots) * b:] == SENTINEL).all()
        return out

    for slots in ((0,), (1, 0), (3, 1, 2), (0, 1, 2, 3)):
        _same(run(slots), np.stack([want[s] for s in slots]), (kind, t, slots))
    other = S.make_net(kind, t, salt=1.5)
    env.critic_load(1, copy.deepcopy(other).to(env.device))
    want1 = S.twin(other, x, which=1)
    assert not np.array_equal(S.words(want1), S.words(want[1]))
    _same(run((0, 1, 2, 3)), np.stack([want[0], want1, want[2], want[3]]), 'slot 1 reloaded')
    env.critic_load(1, dnets[1])
    _same(run((1,)), want[1][None], 'slot 1 restored')


def test_device_critics_repack_per_slot():
    """a forward, an in-place Adam step on net 0, a forward: slot 0 alone re-packs and the result is the twin on the new weights;
    _soft_update into net 1: slot 1 alone re-packs; an unchanged call packs nothing"""
    from hope_amd import ParkingBatch
    from hope_amd import agent_glue as G
    from hope_amd.agents import _soft_update
    kind, t, b = 'sac', 4, 65
    e = ParkingBatch(16, 32)
    nets = [S.make_net(kind, t, salt).to(e.device) for salt in (0.3, 0.5)]
    x = S.inputs(b, kind, t, seed=3)
    nobs, act = S.nobs(x, e.device)
    crit = G.DeviceCritics(e, nets)

    def check(what):
        got = crit(nobs, act)
        assert len(got) == 2 and all(g.shape == (b, 1) and g.dtype == torch.float32 for g in got)
        for g, n in zip(got, nets):
            _same(g[:, 0], S.twin(_cpu(n), x), what)
        return [g.cpu().numpy().copy() for g in got]

    first = check('first')
    assert crit.on_device and crit.packs == [1, 1]
    opt = torch.optim.Adam(nets[0].parameters(), lr=1e-3)
    for i, p in enumerate(nets[0].parameters()):
        p.grad = torch.sin(torch.arange(p.numel(), device=e.device, dtype=torch.float32) + i).view(p.shape)
    opt.step()
    second = check('after the step')
    assert crit.packs == [2, 1]
    assert not np.array_equal(S.words(first[0]), S.words(second[0])) and np.array_equal(S.words(first[1]), S.words(second[1]))
    _soft_update(nets[1], nets[0], 0.25)
    third = check('after the soft update')
    assert crit.packs == [2, 2] and not np.array_equal(S.words(third[1]), S.words(second[1]))
    check('unchanged')
    assert crit.packs == [2, 2]
    _same(crit(nobs, act, which=(1,))[0], third[1], 'one of the two')
    crit.chunk = 32                                                  # longer inputs go through in pieces
    for g, w in zip(crit(nobs, act), third):
        _same(g, w, 'chunked')
    assert crit.packs == [2, 2]
    e.close()


def test_load_and_forward_are_ordered_by_their_stream():
    """torch produces the inputs and the parameters on a side stream, the loads and the forward are enqueued there and the result is
    copied back there: nothing synchronises the host in between"""
    from hope_amd import ParkingBatch
    kind, t, b = 'sac', 5, 129
    nets = [S.make_net(kind, t, salt) for salt in (0.3, 0.5)]
    x = S.inputs(b, kind, t, seed=9, n_nets=2)
    want = np.stack([S.twin(n, x, which=i) for i, n in enumerate(nets)])
    e = ParkingBatch(16, 32)
    e.enable_critics(2, 1, 1, max_batch=b)
    side = torch.cuda.Stream(device=e.device)
    hx = {k: torch.from_numpy(v.copy()).pin_memory() for k, v in x.items()}
    hnets = [copy.deepcopy(n) for n in nets]
    for n in hnets:
        for p in n.parameters():
            p.data = p.data.pin_memory()
    torch.cuda.synchronize(e.device)
    with torch.cuda.stream(side):
        dnets = [copy.deepcopy(n) for n in nets]
        for dn, hn in zip(dnets, hnets):
            for p, q in zip(dn.parameters(), hn.parameters()):
                p.data = (q.data.to(e.device, non_blocking=True) * 2.0) * 0.5
        dx = {k: v.to(e.device, non_blocking=True) for k, v in hx.items()}
        for _ in range(40):                                        # some work in front of the values the calls read
            dx = {k: (v * 2.0) * 0.5 for k, v in dx.items()}
        for s, dn in enumerate(dnets):
            e.critic_load(s, dn)
        got = e.critic_forward((0, 1), dx['lidar'], dx['target'], dx['mask'], dx['img_token'], dx['action']).cpu()
    _same(got, want, 'side stream')
    torch.cuda.synchronize(e.device)
    e.close()


def test_misuse_fails_loudly():
    """HOPE_ESTATE before the enable and for a slot without parameters; HOPE_EINVAL for a bad enable, n = 0 and n > n_slots, a slot
    out of range or named twice, a missing or superfluous action or image token, a NULL or misaligned pointer, a batch of 0 and of
    max_batch + 1, a bad load -- each refused before anything is launched: the slots and the output keep their words"""
    from hope_amd import ParkingBatch
    from hope_amd import _lib as L
    mb, kind, t = 40, 'sac', 4
    e = ParkingBatch(16, 32)
    dev, lib, h = e.device, e.lib, e.h
    nets = [S.make_net(kind, t, salt) for salt in (0.3, 0.5)]
    dnets = [copy.deepcopy(n).to(dev) for n in nets]
    x = S.inputs(mb + 1, kind, t)
    d = {k: torch.from_numpy(v).to(dev) for k, v in x.items() if v is not None}
    out = torch.full((2, mb + 1), float(SENTINEL), device=dev)
    token = torch.zeros((2, mb + 1, 128), device=dev)
    P = lambda q: None if q is None else C.c_void_p(q if isinstance(q, int) else q.data_ptr())  # noqa: E731
    err = lambda: lib.hope_last_error().decode()  # noqa: E731
    params, keep = L.critic_params('hope_env_critic_load', dnets[0], dev)

    def fwd(slots=(0, 1), batch=mb, n=None, **ptr):
        a = {'lidar': d['lidar'], 'target': d['target'], 'mask': d['mask'], 'img_token': None, 'action': d['action'], 'out': out}
        a.update(ptr)
        sl = None if slots is None else (C.c_int * max(len(slots), 1))(*slots)
        return lib.hope_env_critic_forward(h, sl, len(slots or ()) if n is None else n, *(P(a[k]) for k in ('lidar', 'target', 'mask', 'img_token', 'action')),
                                           batch, P(a['out']), e._stream())

    assert lib.hope_env_critic_load(h, 0, C.byref(params), None) == ESTATE and 'hope_env_critic_enable first' in err()
    assert fwd() == ESTATE and 'hope_env_critic_enable first' in err()
    for shape in ((0, 0, 1, mb), (L.CRITIC_SLOTS + 1, 0, 1, mb), (2, 2, 1, mb), (2, 0, -1, mb), (2, 0, 1, 0), (2, 0, 1, L.POLICY_MAX_BATCH + 1)):
        assert lib.hope_env_critic_enable(h, *shape) == EINVAL and err().startswith('hope_env_critic_enable:'), shape
    assert fwd() == ESTATE                                         # a refused enable enabled nothing
    with pytest.raises(ValueError):
        e.enable_critics(5)
    e.enable_critics(2, False, True, max_batch=mb)
    assert fwd() == ESTATE and 'hope_env_critic_load first' in err()
    e.critic_load(0, dnets[0])
    assert fwd() == ESTATE and 'hope_env_critic_load first' in err()       # slot 1 has nothing yet
    assert fwd(slots=(0,)) == 0
    e.critic_load(1, dnets[1])
    want = np.stack([S.twin(n, {k: (None if v is None else v[:mb]) for k, v in x.items()}) for n in nets])
    assert fwd() == 0
    got = out.view(-1)[:2 * mb].view(2, mb)                        # out [n][batch] at batch mb
    _same(got, want, 'good call')
    out.fill_(float(SENTINEL))
    # a load that fails leaves the slot as it is
    assert lib.hope_env_critic_load(h, 0, None, None) == EINVAL and 'null parameter struct' in err()
    assert lib.hope_env_critic_load(h, 2, C.byref(params), None) == EINVAL and lib.hope_env_critic_load(h, -1, C.byref(params), None) == EINVAL
    for field, _ in L.CRITIC_FIELDS[::5]:
        bad = L.CriticParams.from_buffer_copy(params)
        setattr(bad, field, None)
        assert lib.hope_env_critic_load(h, 0, C.byref(bad), None) == EINVAL and 'null tensor' in err(), field
        setattr(bad, field, getattr(params, field) + 2)
        assert lib.hope_env_critic_load(h, 0, C.byref(bad), None) == EINVAL and 'misaligned tensor' in err(), field
    assert fwd(slots=None, n=1) == EINVAL and fwd(slots=(), n=0) == EINVAL and fwd(slots=(0, 1, 0), n=3) == EINVAL
    assert fwd(slots=(0, 2)) == EINVAL and 'outside' in err()
    assert fwd(slots=(-1,)) == EINVAL and 'outside' in err()
    assert fwd(slots=(1, 1)) == EINVAL and 'named twice' in err()
    for k in ('lidar', 'target', 'mask', 'out'):
        assert fwd(**{k: None}) == EINVAL and 'null lidar / target / mask / out' in err(), k
    for k in ('lidar', 'target', 'mask', 'action', 'out'):
        base = out if k == 'out' else d[k]
        assert fwd(**{k: base.data_ptr() + 2}) == EINVAL and 'misaligned buffer' in err(), k
    assert fwd(img_token=token) == EINVAL and 'there is no image token' in err()
    assert fwd(action=None) == EINVAL and 'the action is missing' in err()
    assert fwd(batch=0) == EINVAL and fwd(batch=-1) == EINVAL and fwd(batch=mb + 1) == EINVAL and f'max_batch ({mb})' in err()
    with pytest.raises(L.HopeError, match='lidar must be float32'):
        e.critic_forward((0,), d['lidar'].double(), d['target'], d['mask'], None, d['action'])
    with pytest.raises(ValueError, match='enabled for'):
        e.critic_load(0, S.make_net('ppo', 3).to(dev))
    torch.cuda.synchronize(dev)
    assert (out.cpu().numpy() == SENTINEL).all(), 'a refused call wrote to out'
    assert fwd() == 0
    _same(got, want, 'after the refused calls')                    # the slots hold the loaded words
    # the same shape again keeps the slots and takes the larger max_batch; another shape drops them
    e.enable_critics(2, False, True, max_batch=mb + 1)
    assert fwd(slots=(1,), batch=mb + 1) == 0
    e.enable_critics(2, True, False, max_batch=mb)
    assert fwd(img_token=token, action=None) == ESTATE and 'hope_env_critic_load first' in err()
    pnet = S.make_net('ppo', 4).to(dev)
    e.critic_load(0, pnet).critic_load(1, pnet)
    assert fwd(action=None) == EINVAL and 'the image token is missing' in err()
    assert fwd(img_token=token) == EINVAL and 'there is no action' in err()
    sac_params, keep2 = L.critic_params('hope_env_critic_load', dnets[0], dev)
    assert lib.hope_env_critic_load(h, 0, C.byref(sac_params), None) == EINVAL and 'action tensors must be NULL' in err()
    assert fwd(img_token=token, action=None) == 0
    e.disable_critics()
    assert fwd(img_token=token, action=None) == ESTATE
    e.close()


def test_the_policy_forward_and_the_critics_share_a_handle():
    """enabling and loading either leaves the other's results as they were; the policy forward still refuses five tokens"""
    from hope_amd import ParkingBatch
    b = 33
    e = ParkingBatch(16, 32)
    actor = PS.make_net('actor', 3)
    px = PS.inputs(b, 3, seed=4)
    pwant = PS.twin(actor, px)
    kind, t = 'sac', 5
    nets = [S.make_net(kind, t, salt) for salt in (0.3, 0.5)]
    x = S.inputs(b, kind, t, seed=4, n_nets=2)
    want = np.stack([S.twin(n, x, which=i) for i, n in enumerate(nets)])
    pd = {k: _dev(e, v)[0] for k, v in px.items()}
    d = {k: _dev(e, v)[0] for k, v in x.items()}
    policy = lambda: e.policy_forward(pd['lidar'], pd['target'], pd['mask'])  # noqa: E731
    critics = lambda: e.critic_forward((0, 1), d['lidar'], d['target'], d['mask'], d['img_token'], d['action'])  # noqa: E731
    e.enable_policy(*PS.shape_of(actor), max_batch=b)
    e.policy_load(copy.deepcopy(actor).to(e.device))
    _same(policy(), pwant, 'policy alone')
    e.enable_critics(2, True, True, max_batch=b)
    for s, n in enumerate(nets):
        e.critic_load(s, copy.deepcopy(n).to(e.device))
    _same(critics(), want, 'critics next to the policy')
    _same(policy(), pwant, 'policy next to the critics')
    assert e.lib.hope_env_policy_enable(e.h, 5, 2, 1, b) == EINVAL
    with pytest.raises(ValueError):
        e.enable_policy(n_tokens=5)
    _same(policy(), pwant, 'policy after the refused enable')
    e.disable_policy()
    _same(critics(), want, 'critics without the policy')
    e.enable_policy(*PS.shape_of(actor), max_batch=b)
    e.policy_load(copy.deepcopy(actor).to(e.device))
    e.disable_critics()
    _same(policy(), pwant, 'policy without the critics')
    e.close()


class _TwinCritics:
    """stands in as agent.device_critics: the host twin of each net's present weights on the same inputs"""

    def __init__(self, nets):
        self.nets = list(nets)

    def __call__(self, nobs, action=None, which=None):
        dev = nobs['lidar'].device
        arr = lambda v: None if v is None else np.ascontiguousarray(v.detach().float().cpu().numpy())  # noqa: E731
        x = {'lidar': arr(nobs['lidar']), 'target': arr(nobs['target']), 'mask': arr(nobs['action_mask']), 'img_token': None, 'action': arr(action)}
        return [torch.from_numpy(S.twin(_cpu(self.nets[i]), x)).to(dev).unsqueeze(1) for i in (range(len(self.nets)) if which is None else which)]


def _lots(n, seed=11):
    from hope_amd import ParkingBatch
    from hope_amd.scene_gen import mixed_arrays
    arrs = mixed_arrays(n, levels=('Normal', 'Complex', 'Extrem'), seed=seed, max_obst=32)
    e = ParkingBatch(n, 32)
    e.set_scene_arrays(np.arange(n), *arrs[:5])
    return e


def _params(*nets):
    return [p.detach().cpu().numpy().copy() for n in nets for p in n.parameters()]


@pytest.mark.parametrize('algo', ['sac', 'ppo'])
def test_one_update_with_the_critics_on_the_device(algo):
    """64 scenes, one update of SACTrainer(sac_update='device', critics='device') / PPOTrainer(gae='device', critics='device') against
    the same run whose device_critics calls the host twin: the losses and every parameter behind the update, word for word"""
    from hope_amd import agents as A
    from hope_amd.rollout import PPOTrainer, SACTrainer
    n, runs = 64, {}
    for which in ('device', 'twin'):
        e = _lots(n)
        torch.manual_seed(0)
        if algo == 'sac':
            ag = A.BatchedSAC(device=e.device, use_img=False, lr=1e-3)
            tr = SACTrainer(e, ag, horizon=2, update_every=2, seed=3, sac_update='device', critics='device')
            nets = (ag.actor, ag.critic1, ag.critic2, ag.critic_target1, ag.critic_target2)
        else:
            ag = A.BatchedPPO(device=e.device, use_img=False, lr=1e-3, mini_batch=n * 2, mini_epoch=1)
            tr = PPOTrainer(e, ag, horizon=2, seed=3, gae='device', critics='device')
            nets = (ag.actor, ag.critic, ag.critic_target)
        dc = ag.device_critics
        assert dc is tr.device_critics and dc.on_device
        if which == 'twin':
            ag.device_critics = _TwinCritics(dc.nets)
        losses = [o for o in (tr.step() for _ in range(2)) if o is not None]
        torch.cuda.synchronize(e.device)
        assert tr.updates == 1 and len(losses) == 1 and np.isfinite(losses[0]).all()
        if which == 'device':
            assert dc.packs == [1, 1]
        runs[which] = (np.asarray(losses[0], dtype=np.float64), _params(*nets))
        e.close()
    assert np.array_equal(runs['device'][0], runs['twin'][0]), (runs['device'][0], runs['twin'][0])
    for a, b in zip(runs['device'][1], runs['twin'][1]):
        _same(a, b, 'parameters behind the update')
