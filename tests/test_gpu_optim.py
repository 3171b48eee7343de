"""The optimiser block on the device: k_optim (hope_env_optim_adam / hope_env_optim_polyak) against the host twin word for word on the
programmed cases of tests/optim_cases.py, on real parameter sets and inside one SAC and one PPO update."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_cases as OC  # noqa: E402

pytestmark = pytest.mark.gpu
CPU = torch.device('cpu')


@pytest.fixture(scope='module')
def env():
    from hope_amd import ParkingBatch
    e = ParkingBatch(16, 32)
    yield e
    e.close()


def _groups(hypers):
    from hope_amd import _lib as L
    return [L.OptimGroup(*h) for h in hypers]


def _twin_adam(params, grads, ms, vs, hypers, group_of=None):
    from hope_amd import _lib as L
    table, n, _keep = L.optim_entries(params, grads, ms, vs, group_of, 'hope_optim_adam_host')
    L.check(L.load_library().hope_optim_adam_host(table, n, (L.OptimGroup * len(hypers))(*_groups(hypers)), len(hypers)), 'hope_optim_adam_host')


def _twin_polyak(targets, currents, tau):
    from hope_amd import _lib as L
    table, n, _keep = L.optim_entries(targets, currents, call='hope_optim_polyak_host')
    L.check(L.load_library().hope_optim_polyak_host(table, n, float(tau)), 'hope_optim_polyak_host')


def _twin_reference(p, g, m, v, hp):
    t = [torch.from_numpy(x.copy()) for x in (p, g, m, v)]
    _twin_adam([t[0]], [t[1]], [t[2]], [t[3]], [hp])
    return t[0].numpy(), t[2].numpy(), t[3].numpy()


def _same(got, want, what):
    assert np.array_equal(OC.words(got), OC.words(want)), (what, int((OC.words(got) != OC.words(want)).sum()))


@pytest.mark.parametrize('offsets', [(0,), (1,), (1, 0, 3, 2)], ids=['aligned', 'four bytes past', 'both paths in one launch'])
def test_kernel_equals_the_host_twin_on_the_whole_case_table(env, offsets):
    """every numel, first-step zeros, zero / tiny / huge gradients, one non-finite element, every step count, float64 entries next to
    float32 ones, up to four groups and more than 64 entries to a call, sentinels around every buffer"""
    def adam(params, grads, ms, vs, hypers, group_of):
        env.optim_adam(params, grads, ms, vs, _groups(hypers), group_of)
        torch.cuda.synchronize(env.device)
    assert OC.run_table(adam, env.device, offsets, reference=_twin_reference) == 2


@pytest.mark.parametrize('tau', OC.TAUS)
def test_polyak_kernel_equals_the_host_twin(env, tau):
    cases = []
    for i, n in enumerate(OC.NUMELS + OC.NUMELS + (1, 257, 1025)):
        dtype = np.float64 if i >= 2 * len(OC.NUMELS) else np.float32
        c = OC.random_case(n, 50 + i, dtype)
        if n == 5:
            c['g'][2], c['p'][3] = np.inf, np.nan
        cases.append(({'p': c['p'], 'g': c['g']}, 0 if i < len(OC.NUMELS) else 1 + i % 3))
    dev = [OC.torch_case(c, env.device, off) for c, off in cases]
    env.optim_polyak([v['p'] for v, _ in dev], [v['g'] for v, _ in dev], tau)
    host = [OC.torch_case(c, CPU, off)[0] for c, off in cases]
    _twin_polyak([v['p'] for v in host], [v['g'] for v in host], tau)
    torch.cuda.synchronize(env.device)
    for i, ((d, bufs), h) in enumerate(zip(dev, host)):
        _same(d['p'], h['p'], ('target', i))
        _same(d['g'], h['g'], ('current', i))
        assert all(OC.guards_intact(b, x) for b, x in bufs), i


@pytest.mark.parametrize('n_entries', [64, 65, 129])
def test_more_entries_than_one_launch_holds(env, n_entries):
    from hope_amd import _lib as L
    assert L.OPTIM_CAP == 64
    hs = [OC.hyper(t=2), OC.hyper(lr=1e-3, eps=1e-6, t=5)]
    cases = [OC.random_case(1 + (37 * i) % 1500, 900 + i, np.float64 if i % 9 == 8 else np.float32) for i in range(n_entries)]
    group_of = [i % 2 for i in range(n_entries)]
    dev = [OC.torch_case(c, env.device, i % 4) for i, c in enumerate(cases)]
    env.optim_adam(*[[v[k] for v, _ in dev] for k in 'pgmv'], _groups(hs), group_of)
    host = [OC.torch_case(c, CPU)[0] for c in cases]
    _twin_adam(*[[v[k] for v in host] for k in 'pgmv'], hs, group_of)
    torch.cuda.synchronize(env.device)
    for i, ((d, bufs), h) in enumerate(zip(dev, host)):
        for k in 'pgmv':
            _same(d[k], h[k], (i, k))
        assert all(OC.guards_intact(b, x) for b, x in bufs), i


def test_a_call_on_a_side_stream(env):
    """torch produces the tensors on a side stream, both calls are enqueued there and the results are copied back there"""
    hp = OC.hyper(lr=1e-3, t=1)
    c = OC.random_case(5000, 77)
    side = torch.cuda.Stream(env.device)
    with torch.cuda.stream(side):
        t = {k: torch.from_numpy(x).to(env.device, non_blocking=True) for k, x in c.items()}
        tgt = t['p'].clone()
        env.optim_adam([t['p']], [t['g']], [t['m']], [t['v']], _groups([hp]))
        env.optim_polyak([tgt], [t['p']], 0.25)
        got = {k: x.to('cpu', non_blocking=True) for k, x in t.items()}
        got_t = tgt.to('cpu', non_blocking=True)
    side.synchronize()
    want = _twin_reference(c['p'], c['g'], c['m'], c['v'], hp)
    for k, w in zip('pmv', want):
        _same(got[k], w, k)
    _same(got_t, OC.polyak_reference(c['p'], want[0], 0.25), 'target')


def test_every_refusal_names_its_entry_and_launches_nothing(env):
    from hope_amd import _lib as L
    f32, b32 = OC.torch_case(OC.random_case(64, 1), env.device)
    f64, b64 = OC.torch_case(OC.random_case(4, 2, np.float64), env.device)
    before = [b.clone() for b, _ in b32 + b64]
    cases = OC.refusals(L, f32, f64)
    for label, mode, table, n, groups, n_groups, tau, text in cases:
        if mode == 'adam':
            rc, name = env.lib.hope_env_optim_adam(env.h, table, n, groups, n_groups, env._stream()), 'hope_env_optim_adam'
        else:
            rc, name = env.lib.hope_env_optim_polyak(env.h, table, n, tau, env._stream()), 'hope_env_optim_polyak'
        msg = env.lib.hope_last_error().decode()
        assert rc == -1 and msg.startswith(name + ': ') and text in msg, (label, rc, msg)
    torch.cuda.synchronize(env.device)
    for (b, _), was in zip(b32 + b64, before):
        assert torch.equal(b, was)
    with pytest.raises(ValueError, match='entry 0'):                  # the binding's own check: a CPU tensor is not this env's
        env.optim_adam([torch.zeros(3)], [torch.zeros(3)], [torch.zeros(3)], [torch.zeros(3)], _groups([OC.hyper()]))


def _real_sets():
    from hope_amd import policy as P
    torch.manual_seed(0)
    critic = P.SacCritic(P.critic_configs(use_img=True), 2, True)
    actor = P.HopeNet(P.actor_configs(use_img=False), True)
    log_std = torch.zeros(1, 2, requires_grad=True)
    return critic, actor, log_std


def test_three_steps_on_a_real_parameter_set(env):
    """a SacCritic with image (48 tensors, 943 057 elements) and the PPO actor plus log_std (two param groups), three DeviceAdam steps
    with random gradients through ONE call each, against the same steps on the host twin: every word of p, exp_avg, exp_avg_sq"""
    import types
    from hope_amd import agent_glue as G
    sets = {}
    for where in ('device', 'host'):
        critic, actor, log_std = _real_sets()
        dev = env.device if where == 'device' else CPU
        critic.to(dev), actor.to(dev)
        log_std = log_std.detach().to(dev).requires_grad_()
        e = env if where == 'device' else types.SimpleNamespace(n=1, device=CPU)
        opts = [G.DeviceAdam(e, torch.optim.Adam(critic.parameters(), 1e-3)),
                G.DeviceAdam(e, torch.optim.Adam([{'params': actor.parameters()}, {'params': [log_std], 'lr': 1e-2}], 2.5e-5))]
        assert opts[0].on_device == (where == 'device')
        params = list(critic.parameters()) + list(actor.parameters()) + [log_std]
        assert len(list(critic.parameters())) == 48 and sum(p.numel() for p in critic.parameters()) == 943057
        for step in range(3):
            g = torch.Generator().manual_seed(step)
            for p in params:
                p.grad = (torch.randn(p.shape, generator=g) * 10.0 ** torch.randint(-8, 2, p.shape, generator=g)).to(dev)
            G.step_optimizers(*opts)
        state = [s[k] for o in opts for s in o.state.values() for k in ('exp_avg', 'exp_avg_sq')]
        assert all(float(s['step']) == 3 for o in opts for s in o.state.values())
        sets[where] = [x.detach().cpu() for x in params + state]
    assert len(sets['device']) == len(sets['host']) == 3 * len(params)
    for i, (a, b) in enumerate(zip(sets['device'], sets['host'])):
        _same(a, b, i)


def test_device_actor_and_device_critics_repack_after_a_device_step(env):
    """`packs` goes up by exactly one per net that a DeviceAdam.step() or a DevicePolyak call moved, and by none otherwise"""
    from hope_amd import ParkingBatch
    from hope_amd import agent_glue as G
    from hope_amd import agents as A
    e = ParkingBatch(16, 32)
    torch.manual_seed(0)
    ag = A.BatchedPPO(device=e.device, use_img=False, lr=1e-3)
    actor, crit = G.DeviceActor(e, ag.actor), G.DeviceCritics(e, (ag.critic, ag.critic_target))
    G.make_optimizers('device', e, ag)
    nobs = {'lidar': torch.randn(8, 120, device=e.device), 'target': torch.randn(8, 5, device=e.device),
            'action_mask': torch.ones(8, 42, device=e.device)}
    first = (actor(nobs).clone(), [x.clone() for x in crit(nobs)])
    assert actor.packs == 1 and crit.packs == [1, 1]
    for p in list(ag.actor.parameters()) + [ag.log_std]:
        p.grad = torch.full_like(p, 0.5)
    ag.actor_opt.step()                                               # the actor moved, the critics did not
    second = (actor(nobs).clone(), [x.clone() for x in crit(nobs)])
    assert actor.packs == 2 and crit.packs == [1, 1] and not torch.equal(first[0], second[0]) and torch.equal(first[1][0], second[1][0])
    for p in ag.critic.parameters():
        p.grad = torch.full_like(p, -0.5)
    G.step_optimizers(ag.actor_opt, ag.critic_opt)                    # the actor has gradients still: both move
    third = (actor(nobs).clone(), [x.clone() for x in crit(nobs)])
    assert actor.packs == 3 and crit.packs == [2, 1] and not torch.equal(second[1][0], third[1][0]) and torch.equal(second[1][1], third[1][1])
    ag.soft_update([(ag.critic_target, ag.critic)], 0.5)              # the target alone
    fourth = (actor(nobs).clone(), [x.clone() for x in crit(nobs)])
    assert actor.packs == 3 and crit.packs == [2, 2] and not torch.equal(third[1][1], fourth[1][1]) and torch.equal(third[0], fourth[0])
    ag.actor_opt.zero_grad()
    ag.critic_opt.zero_grad()
    G.step_optimizers(ag.actor_opt, ag.critic_opt)                    # no gradient anywhere: nothing moves, nothing re-packs
    actor(nobs), crit(nobs)
    assert actor.packs == 3 and crit.packs == [2, 2]
    e.close()


class _TwinEnv:
    """an env whose optimiser calls copy the tensors to the host, run the host twin and copy the results back"""

    def __init__(self, env):
        self.n, self.device = env.n, env.device

    def optim_adam(self, params, grads, ms, vs, groups, group_of=None):
        from hope_amd import _lib as L
        host = [[x.detach().cpu() for x in col] for col in (params, grads, ms, vs)]
        table, n, _keep = L.optim_entries(*host, group_of, 'hope_optim_adam_host')
        L.check(L.load_library().hope_optim_adam_host(table, n, (L.OptimGroup * len(groups))(*groups), len(groups)), 'hope_optim_adam_host')
        for c in (0, 2, 3):
            for dst, src in zip((params, grads, ms, vs)[c], host[c]):
                dst.copy_(src)

    def optim_polyak(self, targets, currents, tau):
        host = [[x.detach().cpu() for x in col] for col in (targets, currents)]
        _twin_polyak(host[0], host[1], tau)
        for dst, src in zip(targets, host[0]):
            dst.copy_(src)


def _lots(n, seed=11):
    from hope_amd import ParkingBatch
    from hope_amd.scene_gen import mixed_arrays
    arrs = mixed_arrays(n, levels=('Normal', 'Complex', 'Extrem'), seed=seed, max_obst=32)
    e = ParkingBatch(n, 32)
    e.set_scene_arrays(np.arange(n), *arrs[:5])
    return e


@pytest.mark.parametrize('algo', ['sac', 'ppo'])
def test_one_update_with_the_optimisers_on_the_device(algo):
    """64 scenes, one update of SACTrainer(sac_update='device', critics='device', optimizer='device') / PPOTrainer(gae='device',
    minibatch='device', optimizer='device') against the same run whose optimiser steps are the host twin: the losses, every parameter
    and every word of the optimisers' state"""
    from hope_amd import agent_glue as G
    from hope_amd import agents as A
    from hope_amd.rollout import PPOTrainer, SACTrainer
    n, runs = 64, {}
    for which in ('device', 'twin'):
        e = _lots(n)
        torch.manual_seed(0)
        kind = 'device' if which == 'device' else None
        if algo == 'sac':
            ag = A.BatchedSAC(device=e.device, use_img=False, lr=1e-3)
            tr = SACTrainer(e, ag, horizon=2, update_every=2, seed=3, sac_update='device', critics='device', optimizer=kind)
            nets = (ag.actor, ag.critic1, ag.critic2, ag.critic_target1, ag.critic_target2)
        else:
            ag = A.BatchedPPO(device=e.device, use_img=False, lr=1e-3, mini_batch=n, mini_epoch=2)
            tr = PPOTrainer(e, ag, horizon=2, seed=3, gae='device', minibatch='device', optimizer=kind)
            nets = (ag.actor, ag.critic, ag.critic_target)
        if which == 'twin':
            assert tr.optimizers is None
            G.make_optimizers('device', _TwinEnv(e), ag)
        opts = G.torch_optimizers(ag)
        assert all(isinstance(getattr(ag, k), G.DeviceAdam) and getattr(ag, k).on_device for k in G._OPTIMIZER_NAMES if hasattr(ag, k))
        losses = [o for o in (tr.step() for _ in range(2)) if o is not None]
        torch.cuda.synchronize(e.device)
        assert tr.updates == 1 and len(losses) == 1 and np.isfinite(losses[0]).all()
        assert ag.soft_update.calls == (1 if algo == 'sac' else 2)
        words = [p.detach().cpu() for net in nets for p in net.parameters()] + [ag.log_std.detach().cpu()]
        if algo == 'sac':
            words.append(ag.log_alpha.detach().cpu())
        for o in opts:
            for g in o.param_groups:
                for p in g['params']:
                    if p in o.state:
                        assert float(o.state[p]['step']) == (1 if algo == 'sac' else 4)
                        words += [o.state[p]['exp_avg'].cpu(), o.state[p]['exp_avg_sq'].cpu()]
        runs[which] = (np.asarray(losses[0], dtype=np.float64), words)
        e.close()
    assert np.array_equal(runs['device'][0], runs['twin'][0]), (runs['device'][0], runs['twin'][0])
    assert len(runs['device'][1]) == len(runs['twin'][1]) > 100
    for i, (a, b) in enumerate(zip(runs['device'][1], runs['twin'][1])):
        _same(a, b, i)
