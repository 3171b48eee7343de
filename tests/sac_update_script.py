"""Shared by tests/test_sac_update_core.py (CPU, host twins) and tests/test_gpu_sac_update.py (kernels): the host twins' wrappers over
numpy arrays, the test inputs with their branch census, the torch float64 autograd reference of BatchedSAC.update's expressions, a
restatement of the rule's sums (hope_amd/csrc/hope_sac_core.h) in Python floats, and BatchedSAC.update as it was before the
`update_block` argument."""
import ctypes as C
import math

import numpy as np
import torch

from hope_amd import _lib as L
from ppo_batch_script import HALF_LN_2PI, _exp, tree_sum, ulp32, words  # noqa: F401  (the same hm_exp, trees and word views)

GAMMA = 0.99
TARGET_ENTROPY = -2.0
LOG_ALPHA = math.log(0.01) + 0.0123
SIZES = (1, 2, 63, 64, 65, 129, 4097)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def inputs(b, seed=0):
    """-> dict of float32 arrays (and the float64 scalar log_alpha), drawn so that from 63 items on every branch of the rule occurs:
    raw_d inside, exactly +1, exactly -1, beyond +1, beyond -1 ((item + 2 d) % 5); eps_d zero, far positive, far negative, normal
    ((item // 5) % 4) -- with a mean on a bound a zero eps puts z exactly there; p1 <, >, == p2 (item % 3: the critics at the sampled
    action); qt1 <, > qt2; done 0 and 1."""
    rng = np.random.default_rng(130003 * b + seed)
    i = np.arange(b)
    raw = (0.6 * rng.standard_normal((b, 2))).clip(-0.95, 0.95).astype(np.float32)
    eps = rng.standard_normal((b, 2)).astype(np.float32)
    for d in (0, 1):
        c = (i + 2 * d) % 5
        raw[c == 1, d], raw[c == 2, d] = 1.0, -1.0
        raw[c == 3, d] = (1.0 + rng.random(b)[c == 3] + 1e-3).astype(np.float32)
        raw[c == 4, d] = (-1.0 - rng.random(b)[c == 4] - 1e-3).astype(np.float32)
        m = (i // 5) % 4
        eps[m == 0, d] = 0.0
        eps[m == 1, d] = (3.0 * (1.0 + rng.random(b)[m == 1])).astype(np.float32)
        eps[m == 2, d] = (-3.0 * (1.0 + rng.random(b)[m == 2])).astype(np.float32)
    f = lambda: rng.standard_normal(b).astype(np.float32)  # noqa: E731
    p1 = f()
    p2 = np.where(i % 3 == 0, p1 + np.float32(0.25) + np.abs(f()), np.where(i % 3 == 1, p1 - np.float32(0.25) - np.abs(f()), p1)).astype(np.float32)
    return {'raw': raw, 'log_std': np.array([-0.3, 0.2], np.float32), 'eps': eps, 'q1': f(), 'q2': f(), 'qt1': f(), 'qt2': f(),
            'next_lp': (-1.0 + 0.5 * rng.standard_normal(b)).astype(np.float32), 'reward': f(), 'done': (i % 4 == 1).astype(np.float32),
            'p1': p1, 'p2': p2, 'g_action': (rng.standard_normal((b, 2)) / b).astype(np.float32), 'log_alpha': np.array(LOG_ALPHA, np.float64)}


def census(x):
    """how often each branch of the rule occurs in these inputs"""
    raw = x['raw'].astype(np.float64)
    z = raw.clip(-1, 1) + np.exp(x['log_std'].astype(np.float64)) * x['eps'].astype(np.float64)
    out = {}
    for name, v in (('raw', raw), ('z', z)):
        for d in (0, 1):
            w = v[:, d]
            out.update({f'{name}_{d} < -1': int((w < -1).sum()), f'{name}_{d} == -1': int((w == -1).sum()), f'{name}_{d} inside': int((np.abs(w) < 1).sum()),
                        f'{name}_{d} == +1': int((w == 1).sum()), f'{name}_{d} > +1': int((w > 1).sum())})
    out.update({'p1 < p2': int((x['p1'] < x['p2']).sum()), 'p1 > p2': int((x['p1'] > x['p2']).sum()), 'p1 == p2': int((x['p1'] == x['p2']).sum()),
                'qt1 < qt2': int((x['qt1'] < x['qt2']).sum()), 'qt1 > qt2': int((x['qt1'] > x['qt2']).sum()), 'done 0': int((x['done'] == 0).sum()),
                'done 1': int((x['done'] == 1).sum()), 'eps_0 == 0': int((x['eps'][:, 0] == 0).sum()), 'eps_1 == 0': int((x['eps'][:, 1] == 0).sum())})
    return out


# ---- the host twins over numpy arrays ---------------------------------------------------------------------------------------------
def _p(a):
    return C.c_void_p(a.ctypes.data)


def host_sample(x):
    """-> action [B, 2], lp [B]"""
    b = len(x['raw'])
    out = [np.full((b, 2), 7.0, np.float32), np.full(b, 7.0, np.float32)]
    L.check(L.load_library().hope_sac_sample_host(_p(x['raw']), _p(x['log_std']), _p(x['eps']), b, *map(_p, out)), 'hope_sac_sample_host')
    return out


def host_critic(x, gamma=GAMMA):
    """-> q_target, g_q1, g_q2 [B], losses [2]"""
    b = len(x['q1'])
    out = [np.full(s, 7.0, np.float32) for s in ((b,), (b,), (b,), (2,))]
    L.check(L.load_library().hope_sac_critic_host(*(_p(x[k]) for k in ('q1', 'q2', 'qt1', 'qt2', 'next_lp', 'reward', 'done', 'log_alpha')), gamma, b,
                                                  *map(_p, out)), 'hope_sac_critic_host')
    return out


def host_seed(x):
    """-> s1, s2 [B] for the critics p1, p2 at the sampled action"""
    b = len(x['p1'])
    out = [np.full(b, 7.0, np.float32), np.full(b, 7.0, np.float32)]
    L.check(L.load_library().hope_sac_seed_host(_p(x['p1']), _p(x['p2']), b, *map(_p, out)), 'hope_sac_seed_host')
    return out


def host_policy(x, target_entropy=TARGET_ENTROPY):
    """-> g_raw [B, 2], g_log_std [2], g_log_alpha (float64 scalar array), losses [2]"""
    b = len(x['raw'])
    out = [np.full((b, 2), 7.0, np.float32), np.full(2, 7.0, np.float32), np.full((), 7.0, np.float64), np.full(2, 7.0, np.float32)]
    L.check(L.load_library().hope_sac_policy_host(*(_p(x[k]) for k in ('raw', 'log_std', 'eps', 'p1', 'p2', 'g_action', 'log_alpha')), target_entropy, b,
                                                  *map(_p, out)), 'hope_sac_policy_host')
    return out


def host_all(x):
    return {'sample': host_sample(x), 'critic': host_critic(x), 'seed': host_seed(x), 'policy': host_policy(x)}


# ---- torch's float64 autograd of BatchedSAC.update's own expressions ---------------------------------------------------------------
def torch_reference(x, gamma=GAMMA, target_entropy=TARGET_ENTROPY):
    """The lines of BatchedSAC.update on .double() inputs, differentiated by autograd.  The critics at the sampled action are stood
    in by q_k(a) = p_k + sum_d (a_d - a_d.detach()) J_d with J = -B g_action: their values are p_k exactly, and because the two seeds
    of an item always add up to -1 / B, autograd returns g_action at the sampled action whatever branch of the min is taken.
    -> dict of float64 numpy arrays, and abs_sums = sum |terms| of every sum of the rule"""
    import torch.nn.functional as F
    from hope_amd import policy as P
    b = len(x['raw'])
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).double() for k, v in x.items()}
    col = lambda k: t[k].view(b, 1)  # noqa: E731
    log_alpha = t['log_alpha'].clone().requires_grad_()
    alpha = log_alpha.exp().detach().to(torch.float32).double()               # `.to(reward.dtype)`: the reward is float32
    raw, log_std = t['raw'].clone().requires_grad_(), t['log_std'].view(1, 2).clone().requires_grad_()

    def sample():
        mean = torch.clamp(raw, -1, 1)
        ls = log_std.expand_as(mean)
        a = torch.clamp(mean + ls.exp() * t['eps'], -1, 1)
        return a, P.gaussian_log_prob(mean, ls, a)
    out = {}
    with torch.no_grad():
        a, lp = sample()
        out['action'], out['lp'] = a.numpy(), lp.sum(-1).numpy()
        q_t = torch.min(col('qt1'), col('qt2'))
        q_target = col('reward') + (1 - col('done')) * gamma * (q_t - alpha * col('next_lp'))
        out['q_target'] = q_target.numpy().reshape(b)
    q1, q2 = col('q1').clone().requires_grad_(), col('q2').clone().requires_grad_()
    q1_loss, q2_loss = F.mse_loss(q1, q_target), F.mse_loss(q2, q_target)
    (q1_loss + q2_loss).backward()
    out['g_q1'], out['g_q2'] = q1.grad.numpy().reshape(b), q2.grad.numpy().reshape(b)
    out['critic_losses'] = np.array([float(q1_loss.detach()), float(q2_loss.detach())])
    # the seeds: the gradient of the actor loss at the critic outputs
    p1, p2 = col('p1').clone().requires_grad_(), col('p2').clone().requires_grad_()
    (-torch.min(p1, p2)).mean().backward()
    out['s1'], out['s2'] = p1.grad.numpy().reshape(b), p2.grad.numpy().reshape(b)
    # the policy and the temperature
    a_, lp = sample()
    lp = lp.sum(-1, keepdim=True)
    J = -float(b) * t['g_action']
    lin = ((a_ - a_.detach()) * J).sum(-1, keepdim=True)
    actor_terms = alpha * lp - torch.min(col('p1') + lin, col('p2') + lin)
    actor_loss = actor_terms.mean()
    actor_loss.backward()
    out['g_raw'], out['g_log_std'] = raw.grad.numpy(), log_std.grad.numpy().reshape(2)
    ent = (-lp - target_entropy).detach()
    alpha_loss = (log_alpha.exp() * ent).mean()
    alpha_loss.backward()
    out['g_log_alpha'] = float(log_alpha.grad)
    out['policy_losses'] = np.array([float(actor_loss.detach()), float(alpha_loss.detach())])
    terms = policy_terms(x, target_entropy)                                     # (their sizes only: the slack of the sums' bound)
    a64 = math.exp(float(x['log_alpha']))
    out['abs_sums'] = {'critic_losses': np.array([float(((q1 - q_target) ** 2).sum().detach()) / b, float(((q2 - q_target) ** 2).sum().detach()) / b]),
                       'policy_losses': np.array([float(actor_terms.detach().abs().sum()) / b, a64 * float(ent.abs().sum()) / b]),
                       'g_log_std': np.abs(terms[2:]).sum(1), 'g_log_alpha': a64 * float(ent.abs().sum()) / b}
    return out


# ---- the rule's sums restated -----------------------------------------------------------------------------------------------------
def _alpha(x):
    a64 = _exp(float(x['log_alpha']))
    return a64, float(np.float32(a64))


def critic_terms(x, gamma=GAMMA):
    """su_critic's two terms of every item in Python floats (IEEE double, one rounding per operation) -> float64 [2, B]"""
    f = float
    b = len(x['q1'])
    _, alpha = _alpha(x)
    out = np.zeros((2, b))
    for i in range(b):
        mn = f(x['qt1'][i]) if x['qt1'][i] < x['qt2'][i] else f(x['qt2'][i])
        y = f(x['reward'][i]) + ((1.0 - f(x['done'][i])) * gamma) * (mn - alpha * f(x['next_lp'][i]))
        d1, d2 = f(x['q1'][i]) - y, f(x['q2'][i]) - y
        out[:, i] = (d1 * d1, d2 * d2)
    return out


def policy_terms(x, target_entropy=TARGET_ENTROPY):
    """su_policy's four terms (actor, entropy, log_std 0, log_std 1) of every item in Python floats -> float64 [4, B]"""
    f = float
    b = len(x['raw'])
    ls = [f(x['log_std'][0]), f(x['log_std'][1])]
    sd, var = [_exp(ls[0]), _exp(ls[1])], [_exp(2.0 * ls[0]), _exp(2.0 * ls[1])]
    _, alpha = _alpha(x)
    k = alpha / float(b)
    clamp = lambda v: -1.0 if v < -1.0 else (1.0 if v > 1.0 else v)  # noqa: E731
    out = np.zeros((4, b))
    for i in range(b):
        e, dz, eps = [0.0, 0.0], [0.0, 0.0], [f(x['eps'][i, 0]), f(x['eps'][i, 1])]
        for d in (0, 1):
            m = clamp(f(x['raw'][i, d]))
            z = m + sd[d] * eps[d]
            e[d] = clamp(z) - m
            t = k * (e[d] / var[d])
            dz[d] = f(x['g_action'][i, d]) - t if -1.0 <= z <= 1.0 else 0.0
        lp = ((-(e[0] * e[0]) / (2.0 * var[0]) - ls[0]) - HALF_LN_2PI) + ((-(e[1] * e[1]) / (2.0 * var[1]) - ls[1]) - HALF_LN_2PI)
        mn = f(x['p1'][i]) if x['p1'][i] < x['p2'][i] else f(x['p2'][i])
        out[:, i] = (alpha * lp - mn, -lp - target_entropy, (dz[0] * sd[0]) * eps[0] + k * ((e[0] * e[0]) / var[0] - 1.0),
                     (dz[1] * sd[1]) * eps[1] + k * ((e[1] * e[1]) / var[1] - 1.0))
    return out


def restated_sums(x):
    """-> (critic losses [2] float32, policy losses [2] float32, g_log_std [2] float32, g_log_alpha float64) from the per-item terms
    in Python floats, the chunk tree and the merge tree"""
    n = float(len(x['raw']))
    c = [tree_sum(t) for t in critic_terms(x)]
    p = [tree_sum(t) for t in policy_terms(x)]
    a64, _ = _alpha(x)
    ga = a64 * (p[1] / n)
    return (np.array([c[0] / n, c[1] / n]).astype(np.float32), np.array([p[0] / n, ga]).astype(np.float32), np.array([p[2], p[3]]).astype(np.float32),
            np.array(ga, np.float64))


# ---- BatchedSAC.update as it was before the `update_block` argument ----------------------------------------------------------------
def parent_update(ag, batch, noise=None):
    """the body of BatchedSAC.update without the update_block switch, line for line"""
    import torch.nn.functional as F
    from hope_amd import agents as A
    from hope_amd import dist as D
    st, nst = batch['obs'], batch['next_obs']
    action, reward, done = batch['action'], batch['reward'].view(-1, 1), batch['done'].view(-1, 1)
    alpha = ag.alpha.detach().to(reward.dtype)
    with torch.no_grad():
        na, nlp = ag._sample_action(nst, None if noise is None else noise[0])
        nlp = nlp.sum(-1, keepdim=True)
        q_t = torch.min(ag.critic_target1(nst, na), ag.critic_target2(nst, na))
        q_target = reward + (1 - done) * ag.gamma * (q_t - alpha * nlp)
    q1_loss = F.mse_loss(ag.critic1(st, action), q_target)
    q2_loss = F.mse_loss(ag.critic2(st, action), q_target)
    ag.critic_opt1.zero_grad(set_to_none=True)
    ag.critic_opt2.zero_grad(set_to_none=True)
    (q1_loss + q2_loss).backward()
    cparams = list(ag.critic1.parameters()) + list(ag.critic2.parameters())
    ag.allreduce_bytes += D.allreduce_gradients(cparams)
    ag.critic_opt1.step()
    ag.critic_opt2.step()
    for p in cparams:
        p.requires_grad_(False)
    a_, lp = ag._sample_action(st, None if noise is None else noise[1])
    lp = lp.sum(-1, keepdim=True)
    actor_loss = (alpha * lp - torch.min(ag.critic1(st, a_), ag.critic2(st, a_))).mean()
    ag.actor_opt.zero_grad(set_to_none=True)
    actor_loss.backward()
    ag.allreduce_bytes += D.allreduce_gradients(list(ag.actor.parameters()) + [ag.log_std])
    ag.actor_opt.step()
    for p in cparams:
        p.requires_grad_(True)
    if ag.learn_temperature:
        alpha_loss = (ag.alpha * (-lp - ag.target_entropy).detach()).mean()
        ag.alpha_opt.zero_grad(set_to_none=True)
        alpha_loss.backward()
        ag.allreduce_bytes += D.allreduce_gradients([ag.log_alpha])
        ag.alpha_opt.step()
    A._soft_update(ag.critic_target1, ag.critic1, ag.tau)
    A._soft_update(ag.critic_target2, ag.critic2, ag.tau)
    return float(actor_loss.detach()), float(q1_loss.detach())
