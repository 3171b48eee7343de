"""agent_glue.DeviceAdam / DevicePolyak / step_optimizers / make_optimizers on an env without the library (tests/fake_env.OracleEnv: the
host twins run), and BatchedSAC / BatchedPPO updates through them against the same updates with every optimiser step applied by hand
(tests/optim_cases.adam_reference).  No device."""
import os

import numpy as np
import pytest
import torch

from hope_amd import agent_glue as G
from hope_amd import agents as A
from hope_amd import _lib as L

import optim_cases as OC

_ENV = []


@pytest.fixture
def env():
    if not _ENV:
        from fake_env import OracleEnv
        from hope_amd.scenes import SceneSource
        src = SceneSource(levels=('Normal',), seed=3)
        _ENV.append(OracleEnv([src.draw() for _ in range(4)]))
    return _ENV[0]


class HandAdam:
    """a torch.optim.Adam's surface whose step() is adam_reference applied by hand to the optimiser's own tensors"""

    def __init__(self, optimizer):
        self.optimizer, self.steps = optimizer, 0

    param_groups = property(lambda self: self.optimizer.param_groups)
    state = property(lambda self: self.optimizer.state)

    def zero_grad(self, set_to_none=True):
        self.optimizer.zero_grad(set_to_none=set_to_none)

    def load_state_dict(self, sd):
        self.optimizer.load_state_dict(sd)

    @torch.no_grad()
    def step(self):
        self.steps += 1
        for group in self.optimizer.param_groups:
            for p in group['params']:
                if p.grad is None:
                    continue
                st = self.optimizer.state[p]
                if not st:
                    st['step'], st['exp_avg'], st['exp_avg_sq'] = torch.tensor(0.0), torch.zeros_like(p), torch.zeros_like(p)
                st['step'] += 1
                hp = OC.hyper(group['lr'], group['betas'], group['eps'], int(st['step']))
                flat = lambda x: x.detach().numpy().reshape(-1)  # noqa: E731
                new = OC.adam_reference(flat(p), flat(p.grad), flat(st['exp_avg']), flat(st['exp_avg_sq']), hp)
                for dst, src in zip((p, st['exp_avg'], st['exp_avg_sq']), new):
                    dst.copy_(torch.from_numpy(src).view_as(dst))


class HandPolyak:
    def __init__(self):
        self.calls = 0

    @torch.no_grad()
    def __call__(self, pairs, tau):
        self.calls += 1
        for t, c in pairs:
            for tp, cp in zip(t.parameters(), c.parameters()):
                tp.copy_(torch.from_numpy(OC.polyak_reference(tp.numpy().reshape(-1), cp.numpy().reshape(-1), tau)).view_as(tp))


def _by_hand(agent):
    for name in G._OPTIMIZER_NAMES:
        if hasattr(agent, name):
            setattr(agent, name, HandAdam(getattr(agent, name)))
    agent.soft_update = HandPolyak()
    return agent


def _same_words(a, b):
    return np.array_equal(OC.words(a.detach()), OC.words(b.detach()))


def _params(n=3, seed=0, double_last=False):
    torch.manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(s)) for s in ((5, 7), (7,), (1, 2), (1300,))[:n]]
    if double_last:
        ps.append(torch.nn.Parameter(torch.tensor(-4.6, dtype=torch.float64)))
    return ps


def _set_grads(ps, seed, skip=()):
    g = torch.Generator().manual_seed(seed)
    for i, p in enumerate(ps):
        p.grad = None if i in skip else torch.randn(p.shape, generator=g, dtype=p.dtype)


# ---- DeviceAdam ----------------------------------------------------------------------------------------------------------------------
def test_device_adam_does_what_adam_step_does_to_the_same_objects(env):
    ps, qs = _params(4, double_last=True), _params(4, double_last=True)
    opt = G.DeviceAdam(env, torch.optim.Adam([{'params': ps[:2]}, {'params': ps[2:], 'lr': 1e-3, 'eps': 1e-6}], lr=2.5e-5))
    hand = HandAdam(torch.optim.Adam([{'params': qs[:2]}, {'params': qs[2:], 'lr': 1e-3, 'eps': 1e-6}], lr=2.5e-5))
    assert not opt.on_device and isinstance(opt.optimizer, torch.optim.Adam) and opt.param_groups is opt.optimizer.param_groups
    assert opt.state is opt.optimizer.state and len(opt.state) == 0
    ptrs = [p.data_ptr() for p in ps]
    for step in range(1, 4):
        skip = (1,) if step < 3 else ()                               # a parameter without a gradient: skipped, no state
        _set_grads(ps, step, skip)
        _set_grads(qs, step, skip)
        if step == 3:                                                 # a scheduler's change is honoured
            opt.param_groups[0]['lr'] = hand.param_groups[0]['lr'] = 1e-4
        versions = [p._version for p in ps]
        state_ptrs = {i: (opt.state[p]['exp_avg'].data_ptr(), opt.state[p]['exp_avg_sq'].data_ptr(), opt.state[p]['exp_avg']._version)
                      for i, p in enumerate(ps) if p in opt.state}
        opt.step()
        hand.step()
        for i, (p, q) in enumerate(zip(ps, qs)):
            if i in skip:
                assert p not in opt.state and p._version == versions[i] and _same_words(p, q)
                continue
            st = opt.state[p]
            want_t = step if i != 1 else 1
            assert st['step'].dtype == torch.float32 and st['step'].device.type == 'cpu' and st['step'].shape == () and float(st['step']) == want_t
            assert st['exp_avg'].shape == p.shape and st['exp_avg'].dtype == p.dtype
            assert p.data_ptr() == ptrs[i] and p._version == versions[i] + 1
            if i in state_ptrs:
                assert (st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr()) == state_ptrs[i][:2] and st['exp_avg']._version == state_ptrs[i][2] + 1
            assert _same_words(p, q) and _same_words(st['exp_avg'], hand.state[q]['exp_avg']) and _same_words(st['exp_avg_sq'], hand.state[q]['exp_avg_sq']), (step, i)
    assert opt.steps == 3
    opt.zero_grad()
    assert all(p.grad is None for p in ps)
    opt.step()                                                        # nothing has a gradient: nothing moves
    assert opt.steps == 3 and float(opt.state[ps[0]]['step']) == 3
    extra = torch.nn.Parameter(torch.zeros(3))
    opt.add_param_group({'params': [extra]})
    assert opt.optimizer.param_groups[2]['params'][0] is extra


def test_state_dict_round_trip_into_a_plain_adam_and_back(env):
    ps, qs = _params(3), _params(3)
    dev, plain = G.DeviceAdam(env, torch.optim.Adam(ps, lr=1e-3)), torch.optim.Adam(qs, lr=1e-3)
    for step in range(2):
        _set_grads(ps, step)
        dev.step()
    plain.load_state_dict(dev.state_dict())
    for p, q in zip(ps, qs):
        assert float(plain.state[q]['step']) == 2 and _same_words(plain.state[q]['exp_avg_sq'], dev.state[p]['exp_avg_sq'])
        with torch.no_grad():
            q.copy_(p)
    _set_grads(qs, 7)
    plain.step()                                                      # torch goes on from the device path's state
    assert float(plain.state[qs[0]]['step']) == 3
    rs = _params(3)
    back = G.DeviceAdam(env, torch.optim.Adam(rs, lr=1e-3))
    back.load_state_dict(plain.state_dict())
    _set_grads(rs, 8)
    back.step()                                                       # and the device path from torch's
    assert float(back.state[rs[0]]['step']) == 4 and float(back.state[rs[2]]['step']) == 4


@pytest.mark.parametrize('option', ['amsgrad', 'maximize', 'capturable', 'differentiable', 'weight_decay', 'lr', 'sparse gradient', 'optimizer', 'closure'])
def test_every_refused_option_by_name(env, option):
    ps = _params(2)
    make = {'amsgrad': lambda: torch.optim.Adam(ps, amsgrad=True), 'maximize': lambda: torch.optim.Adam(ps, maximize=True),
            'capturable': lambda: torch.optim.Adam(ps, capturable=True), 'differentiable': lambda: torch.optim.Adam(ps, differentiable=True),
            'weight_decay': lambda: torch.optim.Adam(ps, weight_decay=0.01), 'lr': lambda: torch.optim.Adam(ps, lr=torch.tensor(1e-3)),
            'optimizer': lambda: torch.optim.AdamW(ps)}
    if option in make:
        with pytest.raises(ValueError, match='^' + option):
            G.DeviceAdam(env, make[option]())
        if option in ('amsgrad', 'weight_decay'):                     # also when it is switched on later: refused before anything moves
            opt = G.DeviceAdam(env, torch.optim.Adam(ps))
            _set_grads(ps, 1)
            opt.step()
            opt.param_groups[0][option] = True if option == 'amsgrad' else 0.1
            before = [p.detach().clone() for p in ps]
            with pytest.raises(ValueError, match='^' + option):
                G.step_optimizers(G.DeviceAdam(env, torch.optim.Adam(_params(1))), opt)
            assert all(torch.equal(a, p) for a, p in zip(before, ps)) and float(opt.state[ps[0]]['step']) == 1
        return
    opt = G.DeviceAdam(env, torch.optim.Adam(ps))
    _set_grads(ps, 1)
    if option == 'closure':
        with pytest.raises(ValueError, match='^closure'):
            opt.step(lambda: 0.0)
        return
    ps[0].grad = ps[0].grad.to_sparse()
    with pytest.raises(ValueError, match='^sparse gradient'):
        opt.step()
    assert len(opt.state) == 0


def test_step_optimizers_calls_plain_and_mixed_optimisers_in_order(env):
    log = []

    class Rec(torch.optim.Adam):
        def step(self, closure=None):
            log.append(self)
            return super().step(closure)
    ps = _params(4)
    for p in ps:
        p.grad = torch.ones_like(p)
    a, b = Rec([ps[0]]), Rec([ps[1]])
    G.step_optimizers(a, b)
    assert log == [a, b]
    d = G.DeviceAdam(env, torch.optim.Adam([ps[2]]))
    G.step_optimizers(b, d, a)                                        # a mix: each .step() in turn
    assert log == [a, b, b, a] and d.steps == 1 and float(d.state[ps[2]]['step']) == 1
    G.step_optimizers()
    # DeviceAdams over one env: one call of the library for all of them
    calls = []
    lib = d._lib

    class Spy:
        def __getattr__(self, name):
            f = getattr(lib, name)
            return (lambda *a: (calls.append((name, a[1])), f(*a))[1]) if name.startswith('hope_optim') else f
    e = G.DeviceAdam(env, torch.optim.Adam([{'params': [ps[3]]}, {'params': [ps[0]], 'lr': 1e-4}]))
    d._lib = e._lib = Spy()
    G.step_optimizers(d, e)
    assert calls == [('hope_optim_adam_host', 3)] and d.steps == 2 and e.steps == 1
    # five distinct groups: two calls
    calls.clear()
    many = [G.DeviceAdam(env, torch.optim.Adam([torch.nn.Parameter(torch.zeros(2))], lr=10.0 ** -k)) for k in range(5)]
    for o in many:
        o._lib = d._lib
        o.param_groups[0]['params'][0].grad = torch.ones(2)
    G.step_optimizers(*many)
    assert calls == [('hope_optim_adam_host', 4), ('hope_optim_adam_host', 1)]
    other = G.DeviceAdam(_other_env(env), torch.optim.Adam([ps[1]]))
    calls.clear()
    other._lib = d._lib
    G.step_optimizers(d, other)                                       # two envs: each on its own
    assert [c[1] for c in calls] == [1, 1]


def _other_env(env):
    import types
    return types.SimpleNamespace(n=env.n, device=env.device)


def test_device_polyak_is_one_call_for_all_pairs(env):
    torch.manual_seed(1)
    nets = [torch.nn.Linear(9, 5) for _ in range(4)]
    hand = [torch.nn.Linear(9, 5) for _ in range(4)]
    for a, b in zip(nets, hand):
        b.load_state_dict(a.state_dict())
    pol = G.DevicePolyak(env)
    versions = [[p._version for p in n.parameters()] for n in nets]
    pol.polyak([(nets[0], nets[1]), (nets[2], nets[3])], 0.1)
    HandPolyak()([(hand[0], hand[1]), (hand[2], hand[3])], 0.1)
    assert pol.calls == 1 and not pol.on_device
    for i, (a, b) in enumerate(zip(nets, hand)):
        assert all(_same_words(p, q) for p, q in zip(a.parameters(), b.parameters()))
        assert [p._version for p in a.parameters()] == [v + (i % 2 == 0) for v in versions[i]]      # the targets' counters, not the nets'
    with pytest.raises(ValueError, match='parameters'):
        pol.polyak([(nets[0], torch.nn.Linear(9, 5, bias=False))], 0.1)
    with pytest.raises(L.HopeError, match='tau must be in'):
        pol.polyak([(nets[0], nets[1])], 1.5)


# ---- the agents ------------------------------------------------------------------------------------------------------------------------
def _count_forwards(agent, nets):
    counts = {k: 0 for k in nets}
    for k in nets:
        getattr(agent, k).register_forward_hook(lambda *_a, k=k: counts.__setitem__(k, counts[k] + 1))
    return counts


def _opt_steps(agent):
    out = {}
    for name in G._OPTIMIZER_NAMES:
        o = getattr(agent, name, None)
        if o is not None:
            o = getattr(o, 'optimizer', o)
            out[name] = sorted({int(s['step']) for s in o.state.values()})
    return out


def _state_words(agent):
    out = []
    for name in G._OPTIMIZER_NAMES:
        o = getattr(agent, name, None)
        if o is None:
            continue
        o = getattr(o, 'optimizer', o)
        for g in o.param_groups:
            for p in g['params']:
                out.append(OC.words(p.detach()))
                if p in o.state:                                      # (a parameter that never had a gradient has none)
                    out += [OC.words(o.state[p]['exp_avg']), OC.words(o.state[p]['exp_avg_sq'])]
    for name in ('critic_target', 'critic_target1', 'critic_target2'):
        if hasattr(agent, name):
            out += [OC.words(p.detach()) for p in getattr(agent, name).parameters()]
    return out


def _sac(env, kind, seed=0):
    import test_sac_update_core as TS
    ag = TS._agent(1e-3, seed=seed)
    ag.update_block = G.DeviceSacUpdate(env)
    if kind == 'device':
        made = G.make_optimizers('device', env, ag)
        assert sorted(made) == ['actor_opt', 'alpha_opt', 'critic_opt1', 'critic_opt2'] and all(isinstance(o, G.DeviceAdam) for o in made.values())
        assert isinstance(ag.soft_update, G.DevicePolyak)
    elif kind == 'hand':
        _by_hand(ag)
    else:
        assert G.make_optimizers(None, env, ag) is None and not hasattr(ag, 'soft_update')
    return ag


def test_sac_update_with_device_optimizers_equals_the_steps_by_hand(env):
    import test_sac_update_core as TS
    batch = TS._ring_batch()
    torch.manual_seed(5)
    noise = [(torch.randn(10, 2), torch.randn(10, 2)) for _ in range(2)]
    runs, counts = {}, {}
    for kind in ('plain', 'device', 'hand'):
        ag = runs[kind] = _sac(env, kind)
        counts[kind] = _count_forwards(ag, ('actor', 'critic1', 'critic2', 'critic_target1', 'critic_target2'))
        ag.losses = [ag._update_with_block(batch, noise=n) for n in noise]
    assert counts['device'] == counts['plain'] == counts['hand'] == {'actor': 4, 'critic1': 4, 'critic2': 4, 'critic_target1': 2, 'critic_target2': 2}
    assert _opt_steps(runs['device']) == _opt_steps(runs['plain']) == {k: [2] for k in ('actor_opt', 'critic_opt1', 'critic_opt2', 'alpha_opt')}
    assert runs['device'].soft_update.calls == runs['hand'].soft_update.calls == 2        # both targets in one call per update
    assert runs['device'].losses == runs['hand'].losses
    dev, hand = _state_words(runs['device']), _state_words(runs['hand'])
    assert len(dev) == len(hand) and all(np.array_equal(a, b) for a, b in zip(dev, hand))
    assert runs['device'].log_alpha.dtype == torch.float64 and float(runs['device'].log_alpha.detach()) != float(np.log(0.01))
    # the torch path lands within rounding of it
    for a, b in zip(runs['plain'].critic1.parameters(), runs['device'].critic1.parameters()):
        assert float((a.detach() - b.detach()).abs().max()) < 1e-5


def _ppo_inputs(n=4, t=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    obs = {'lidar': torch.randn(n, t, 120, generator=g), 'target': torch.randn(n, t, 5, generator=g),
           'action_mask': (torch.rand(n, t, 42, generator=g) > 0.3).float()}
    last = {k: v[:, 0].clone() for k, v in obs.items()}
    action = torch.randn(n, t, 2, generator=g).clamp(-1, 1)
    reward, done = torch.randn(n, t, generator=g), (torch.rand(n, t, generator=g) < 0.2).float()
    old_lp = -torch.rand(n, t, 2, generator=g)
    perms = [torch.randperm(n * t, generator=g) for _ in range(2)]
    return (obs, action, reward, done, old_lp, last), perms


def _ppo(env, kind):
    torch.manual_seed(0)
    ag = A.BatchedPPO(device='cpu', use_img=False, lr=1e-3, mini_batch=5, mini_epoch=2, state_norm=False)
    if kind == 'device':
        assert sorted(G.make_optimizers('device', env, ag)) == ['actor_opt', 'critic_opt']
    elif kind == 'hand':
        _by_hand(ag)
    return ag


def test_ppo_update_with_device_optimizers_equals_the_steps_by_hand(env):
    args, perms = _ppo_inputs()
    runs, counts = {}, {}
    for kind in ('plain', 'device', 'hand'):
        ag = runs[kind] = _ppo(env, kind)
        counts[kind] = _count_forwards(ag, ('actor', 'critic', 'critic_target'))
        before = [p.detach().clone() for p in ag.critic_target.parameters()]
        versions = [p._version for p in ag.critic_target.parameters()]
        ag.losses = ag.update(*args, perms=perms)
        assert sum(not torch.equal(a, p) for a, p in zip(before, ag.critic_target.parameters())) >= 20
        if kind == 'device':                                          # the target moves once per epoch, not after every step
            assert ag.soft_update.calls == 2 and [p._version for p in ag.critic_target.parameters()] == [v + 2 for v in versions]
    assert counts['device'] == counts['plain'] == counts['hand']
    assert _opt_steps(runs['device']) == _opt_steps(runs['plain']) == {'actor_opt': [6], 'critic_opt': [6]}      # 3 minibatches x 2 epochs
    assert runs['hand'].soft_update.calls == 2 and runs['hand'].actor_opt.steps == 6
    assert runs['device'].losses == runs['hand'].losses
    dev, hand = _state_words(runs['device']), _state_words(runs['hand'])
    assert len(dev) == len(hand) and all(np.array_equal(a, b) for a, b in zip(dev, hand))
    assert _same_words(runs['device'].log_std, runs['hand'].log_std)


def test_a_checkpoint_saved_from_one_path_loads_into_the_other(env, tmp_path):
    from hope_amd.checkpoint import load_hope_checkpoint
    args, perms = _ppo_inputs()

    def save(ag, path):
        torch.save({'actor_net': ag.actor.state_dict(), 'critic_net': ag.critic.state_dict(), 'critic_target': ag.critic_target.state_dict(),
                    'log': ag.log_std.detach(), 'optimizer': G.torch_optimizers(ag)}, path)

    def load(ag, path):
        ck = load_hope_checkpoint(path)
        ag.actor.load_state_dict(ck['state_dicts']['actor_net'])
        ag.critic.load_state_dict(ck['state_dicts']['critic_net'])
        ag.critic_target.load_state_dict(ck['state_dicts']['critic_target'])
        with torch.no_grad():
            ag.log_std.copy_(ck['log_std'])
        saved = ck['raw']['optimizer']
        assert all(type(o) is torch.optim.Adam for o in saved)       # torch objects, whichever path wrote them
        ag.actor_opt.load_state_dict(saved[0].state_dict())
        ag.critic_opt.load_state_dict(saved[1].state_dict())
    for src, dst in (('device', 'plain'), ('plain', 'device'), ('device', 'hand')):
        a, b = _ppo(env, src), _ppo(env, dst)
        a.update(*args, perms=perms)
        path = os.path.join(tmp_path, f'{src}.pt')
        save(a, path)
        load(b, path)
        assert all(np.array_equal(x, y) for x, y in zip(_state_words(a), _state_words(b))) and _opt_steps(b) == {'actor_opt': [6], 'critic_opt': [6]}
        b.update(*args, perms=perms)                                  # and goes on from there
        assert _opt_steps(b) == {'actor_opt': [12], 'critic_opt': [12]}
        if dst == 'hand':                                             # a device run resumed equals the same run resumed by hand
            a.update(*args, perms=perms)
            assert all(np.array_equal(x, y) for x, y in zip(_state_words(a), _state_words(b)))


def test_trainers_take_the_optimizer_argument(env):
    from hope_amd.rollout import PPOTrainer, SACTrainer
    torch.manual_seed(0)
    ag = A.BatchedPPO(device='cpu', use_img=False, lr=1e-4, mini_batch=8, mini_epoch=1)
    tr = PPOTrainer(env, ag, horizon=2, seed=1, optimizer='device')
    assert isinstance(ag.actor_opt, G.DeviceAdam) and tr.optimizers['critic_opt'] is ag.critic_opt
    out = [tr.step() for _ in range(2)]
    assert out[1] is not None and np.isfinite(out[1]).all() and ag.actor_opt.steps == 1 and ag.soft_update.calls == 1
    sac = A.BatchedSAC(device='cpu', use_img=False, lr=1e-4, batch_size=8)
    ts = SACTrainer(env, sac, horizon=2, update_every=1, seed=1, optimizer='device')
    out = [ts.step() for _ in range(3)]
    assert ts.updates == 2 and sac.alpha_opt.steps == 2 and sac.soft_update.calls == 2 and np.isfinite(out[-1]).all()
    plain = A.BatchedSAC(device='cpu', use_img=False, batch_size=8)
    tp = SACTrainer(env, plain, horizon=2, seed=1)
    assert tp.optimizers is None and type(plain.critic_opt1) is torch.optim.Adam and not hasattr(plain, 'soft_update')
    with pytest.raises(ValueError, match='optimizer must be'):
        PPOTrainer(env, A.BatchedPPO(device='cpu', use_img=False), optimizer='gpu')
    with pytest.raises(ValueError, match='needs an agent'):
        G.make_optimizers('device', env, object())
