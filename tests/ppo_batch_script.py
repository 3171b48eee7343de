"""Shared by tests/test_ppo_batch_core.py (CPU, host twins) and tests/test_gpu_ppo_batch.py (kernels): the host twins' wrappers over numpy
arrays, the test inputs, the torch float64 reference of the loss, and a restatement of the rule's sums (hope_amd/csrc/hope_ppo_core.h):
the per-item terms in Python floats with an exact fused multiply-add, the chunk tree and the merge tree."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import torch

from hope_amd import _lib as L

CHUNK = 64
CLIP = 0.2
HALF_LN_2PI = 0.9189385332046727
RING_KEYS = (('lidar', 120), ('target', 5), ('action_mask', 42), ('action', 2), ('log_prob', 2))
OUT_KEYS = (('lidar', 120), ('target', 5), ('mask', 42), ('action', 2), ('old_lp', None), ('adv', None), ('v_target', None))


def words(a):
    """the raw words of a float32 / int32 / float64 array"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


# ---- gather ---------------------------------------------------------------------------------------------------------------------
def ring_arrays(n, t, seed=0):
    """-> the ring's seven float32 arrays ([n, t, width] / [n, t]) and adv, v_target [n t]: every word different"""
    rng = np.random.default_rng(7919 * n + 31 * t + seed)
    r = {k: rng.standard_normal((n, t, w)).astype(np.float32) for k, w in RING_KEYS}
    r['reward'], r['done'] = rng.standard_normal((n, t)).astype(np.float32), (rng.random((n, t)) < 0.2).astype(np.float32)
    return r, rng.standard_normal(n * t).astype(np.float32), rng.standard_normal(n * t).astype(np.float32)


def ring_struct(r):
    """the hope_ring_t over the numpy arrays of ring_arrays (hold them while it is used)"""
    n, t = r['reward'].shape
    return L.Ring(n=n, T=t, **{k: r[k].ctypes.data for k in ('lidar', 'target', 'action_mask', 'action', 'log_prob', 'reward', 'done')})


def batch_arrays(mb, fill=7.0):
    """-> the eight output arrays of a gathered minibatch, prefilled"""
    o = {k: np.full((mb,) if w is None else (mb, w), fill, np.float32) for k, w in OUT_KEYS}
    o['idx'] = np.full(mb, 7, np.int32)
    return o


def batch_struct(o):
    return L.PpoBatch(**{k: v.ctypes.data for k, v in o.items()})


def host_gather(r, adv, v_target, index):
    """hope_ppo_gather_host over numpy arrays; index: an int64 array, contiguous (it may be a view at an offset) -> the eight outputs"""
    index = np.asarray(index)
    assert index.dtype == np.int64 and index.flags.c_contiguous
    o = batch_arrays(len(index))
    L.check(L.load_library().hope_ppo_gather_host(ring_struct(r), adv.ctypes.data, v_target.ctypes.data, index.ctypes.data, len(index), batch_struct(o)),
            'hope_ppo_gather_host')
    return o


def torch_gather(r, adv, v_target, index):
    """what BatchedPPO.update's torch path reads for the same index (in range): obs[k].reshape(m, ...)[ri] and its neighbours"""
    n, t = r['reward'].shape
    ri = torch.from_numpy(np.ascontiguousarray(index))
    flat = {k: torch.from_numpy(r[k]).reshape((n * t,) + r[k].shape[2:]) for k, _ in RING_KEYS}
    return {'lidar': flat['lidar'][ri].numpy(), 'target': flat['target'][ri].numpy(), 'mask': flat['action_mask'][ri].numpy(),
            'action': flat['action'][ri].numpy(), 'old_lp': flat['log_prob'].sum(1, keepdim=True)[ri].numpy().reshape(-1),
            'adv': torch.from_numpy(adv).reshape(-1, 1)[ri].numpy().reshape(-1), 'v_target': torch.from_numpy(v_target).reshape(-1, 1)[ri].numpy().reshape(-1),
            'idx': ri.numpy().astype(np.int32)}


# ---- loss -----------------------------------------------------------------------------------------------------------------------
def loss_inputs(mb, seed=0, clip=CLIP):
    """-> dict of float32 arrays raw [mb, 2], log_std [2], value [mb], action [mb, 2], old_lp, adv, v_target [mb], drawn so that with a
    period of 45 items every branch of the rule occurs: the ratio below lo / inside / above hi (item % 3), adv negative / positive /
    zero ((item // 3) % 3), raw_0 inside, exactly +1, exactly -1, beyond +1, beyond -1 ((item // 9) % 5; raw_1 one class further)"""
    rng = np.random.default_rng(104729 * mb + seed)
    i = np.arange(mb)
    log_std = np.array([-0.3, 0.2], np.float32)
    raw = (0.6 * rng.standard_normal((mb, 2))).clip(-0.95, 0.95).astype(np.float32)
    for d in (0, 1):
        c = (i // 9 + d) % 5
        raw[c == 1, d], raw[c == 2, d] = 1.0, -1.0
        raw[c == 3, d] = (1.0 + rng.random(mb)[c == 3] + 1e-3).astype(np.float32)
        raw[c == 4, d] = (-1.0 - rng.random(mb)[c == 4] - 1e-3).astype(np.float32)
    mean = raw.astype(np.float64).clip(-1, 1)
    std = np.exp(log_std.astype(np.float64))
    action = (mean + std * rng.standard_normal((mb, 2))).clip(-1, 1).astype(np.float32)
    var = np.exp(2.0 * log_std.astype(np.float64))
    lp = (-((action - mean) ** 2) / (2.0 * var) - log_std - HALF_LN_2PI).sum(1)
    target = np.where(i % 3 == 0, 1.0 - clip - 0.05 - 0.4 * rng.random(mb), np.where(i % 3 == 1, 1.0 + (clip - 0.02) * (2 * rng.random(mb) - 1),
                                                                                    1.0 + clip + 0.05 + rng.random(mb)))
    old_lp = (lp - np.log(target)).astype(np.float32)
    adv = rng.standard_normal(mb).astype(np.float32)
    adv = np.where((i // 3) % 3 == 0, -np.abs(adv) - 1e-3, np.where((i // 3) % 3 == 1, np.abs(adv) + 1e-3, 0.0)).astype(np.float32)
    return {'raw': raw, 'log_std': log_std, 'value': rng.standard_normal(mb).astype(np.float32), 'action': action, 'old_lp': old_lp, 'adv': adv,
            'v_target': rng.standard_normal(mb).astype(np.float32)}


def host_loss(x, clip=CLIP):
    """hope_ppo_loss_host over the arrays of loss_inputs -> g_raw [mb, 2], g_log_std [2], g_value [mb], losses [2] (float32)"""
    x = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in x.items()}
    mb = len(x['value'])
    b = L.PpoBatch(action=x['action'].ctypes.data, old_lp=x['old_lp'].ctypes.data, adv=x['adv'].ctypes.data, v_target=x['v_target'].ctypes.data)
    out = [np.full(s, 7.0, np.float32) for s in ((mb, 2), (2,), (mb,), (2,))]
    L.check(L.load_library().hope_ppo_loss_host(x['raw'].ctypes.data, x['log_std'].ctypes.data, x['value'].ctypes.data, b, mb, clip,
                                                *(a.ctypes.data for a in out)), 'hope_ppo_loss_host')
    return out


def torch_reference(x, clip=CLIP):
    """the lines of BatchedPPO.update on .double() inputs, differentiated by autograd -> dict: g_raw, g_log_std, g_value, losses (float64
    numpy), the ratio and the two sides of the min per item, and abs_sums = sum |terms| of {actor, critic, log_std 0, log_std 1}"""
    import torch.nn.functional as F
    from hope_amd import policy as P
    mb = len(x['value'])
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).double() for k, v in x.items()}
    raw, value, log_std = t['raw'].requires_grad_(), t['value'].view(mb, 1).requires_grad_(), t['log_std'].view(1, 2).requires_grad_()
    mean = torch.clamp(raw, -1, 1)
    lp = P.gaussian_log_prob(mean, log_std.expand_as(mean), t['action']).sum(1, keepdim=True)
    lp.retain_grad()
    ratio = (lp - t['old_lp'].view(mb, 1)).exp()
    a = t['adv'].view(mb, 1)
    u, c = ratio * a, torch.clamp(ratio, 1 - clip, 1 + clip) * a
    terms = -torch.min(u, c)
    actor_loss = terms.mean()
    critic_loss = F.mse_loss(value, t['v_target'].view(mb, 1))
    (actor_loss + critic_loss).backward()
    with torch.no_grad():
        e2v = (t['action'] - mean) ** 2 / torch.exp(2.0 * log_std)
        ls_terms = lp.grad * (e2v - 1.0)
        abs_sums = np.array([float(terms.abs().sum()) / mb, float(((value - t['v_target'].view(mb, 1)) ** 2).sum()) / mb,
                             float(ls_terms[:, 0].abs().sum()), float(ls_terms[:, 1].abs().sum())])
    return {'g_raw': raw.grad.numpy(), 'g_log_std': log_std.grad.numpy().reshape(2), 'g_value': value.grad.numpy().reshape(mb),
            'losses': np.array([float(actor_loss.detach()), float(critic_loss.detach())]), 'ratio': ratio.detach().numpy().reshape(mb),
            'u': u.detach().numpy().reshape(mb), 'c': c.detach().numpy().reshape(mb), 'abs_sums': abs_sums}


def ulp32(x):
    """one unit in the last place of float32 at |x| (float64 array)"""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def census(x, ref, clip=CLIP):
    """how often each branch of the rule occurs in these inputs"""
    lo, hi, a, raw = 1 - clip, 1 + clip, x['adv'].astype(np.float64), x['raw']
    r = ref['ratio']
    out = {'a == 0': int((a == 0).sum()), 'raw == +1': int((raw == 1).sum()), 'raw == -1': int((raw == -1).sum()), 'raw > +1': int((raw > 1).sum()),
           'raw < -1': int((raw < -1).sum()), 'raw inside': int((np.abs(raw) < 1).sum())}
    for name, m in (('ratio < lo', r < lo), ('ratio > hi', r > hi), ('ratio inside', (r >= lo) & (r <= hi))):
        out[name + ', a < 0'], out[name + ', a > 0'] = int((m & (a < 0)).sum()), int((m & (a > 0)).sum())
    return out


# ---- the rule's sums restated -----------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """a * b + c rounded once (int / int division is correctly rounded)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _exp(x):
    """hope_math.h's hm_exp, operation for operation (|x| <= 700)"""
    kd = float(round(x * 1.4426950408889634))              # rint: to nearest, ties to even
    r = _fma(-kd, 0.6931471803691238, x)
    r = _fma(-kd, 1.9082149288430703e-10, r)
    r = _fma(-kd, 4.275175589747649e-20, r)
    p = 1.1470745597729725e-11
    for k in (1.6059043836821613e-10, 2.08767569878681e-09, 2.505210838544172e-08, 2.755731922398589e-07, 2.7557319223985893e-06, 2.48015873015873e-05,
              0.0001984126984126984, 0.001388888888888889, 0.008333333333333333, 0.041666666666666664, 0.16666666666666666, 0.5):
        p = _fma(p, r, k)
    return math.ldexp(1.0 + _fma(r, r * p, r), int(kd))


def item_terms(x, clip=CLIP):
    """pb_item's four terms of every item in Python floats (IEEE double, one rounding per operation) -> float64 [4, mb]"""
    f = lambda v: float(v)  # noqa: E731  (float32 -> double: exact)
    mb = len(x['value'])
    ls = [f(x['log_std'][0]), f(x['log_std'][1])]
    var = [_exp(2.0 * ls[0]), _exp(2.0 * ls[1])]
    n, lo, hi = float(mb), 1.0 - clip, 1.0 + clip
    out = np.zeros((4, mb))
    for i in range(mb):
        e = [f(x['action'][i, d]) - min(max(f(x['raw'][i, d]), -1.0), 1.0) for d in (0, 1)]
        lp = ((-(e[0] * e[0]) / (2.0 * var[0]) - ls[0]) - HALF_LN_2PI) + ((-(e[1] * e[1]) / (2.0 * var[1]) - ls[1]) - HALF_LN_2PI)
        ratio = _exp(lp - f(x['old_lp'][i]))
        a = f(x['adv'][i])
        u = ratio * a
        c = (lo if ratio < lo else (hi if ratio > hi else ratio)) * a
        wu = 1.0 if u < c else (0.0 if u > c else 0.5)
        dmin = a * (wu + (1.0 - wu) * (1.0 if lo <= ratio <= hi else 0.0))
        k = -(dmin * ratio) / n
        dv = f(x['value'][i]) - f(x['v_target'][i])
        out[:, i] = (-(u if u < c else c), dv * dv, k * ((e[0] * e[0]) / var[0] - 1.0), k * ((e[1] * e[1]) / var[1] - 1.0))
    return out


def tree_sum(terms):
    """64-item chunks padded with +0.0 and combined by the aligned tree, the chunk partials by the aligned tree with pass-through"""
    mb = len(terms)
    nk = (mb + CHUNK - 1) // CHUNK
    c = np.zeros(nk * CHUNK)
    c[:mb] = terms
    c = c.reshape(nk, CHUNK)
    h = 1
    while h < CHUNK:
        c[:, 0::2 * h] = c[:, 0::2 * h] + c[:, h::2 * h]
        h *= 2
    p = c[:, 0].copy()
    h = 1
    while h < nk:
        for i in range(0, nk - h, 2 * h):
            p[i] = p[i] + p[i + h]
        h *= 2
    return p[0]


def restated_sums(x, clip=CLIP):
    """-> (g_log_std [2], losses [2]) float32, from item_terms and tree_sum"""
    t = item_terms(x, clip)
    s = [tree_sum(t[q]) for q in range(4)]
    mb = float(len(x['value']))
    return np.array([s[2], s[3]]).astype(np.float32), np.array([s[0] / mb, s[1] / mb]).astype(np.float32)


# ---- BatchedPPO.update as it was before the `minibatch` argument ------------------------------------------------------------------
def parent_update(ag, obs, action, reward, done, old_log_prob, last_obs, perms):
    """the body of BatchedPPO.update without the minibatch switch, line for line"""
    import torch.nn.functional as F
    from hope_amd import agents as A
    from hope_amd import dist as D
    from hope_amd import policy as P
    adv, v_target = ag.advantages(obs, reward, done, last_obs)
    n, t = reward.shape
    m = n * t
    flat = {k: v.reshape((m,) + v.shape[2:]) for k, v in obs.items()}
    action, old_lp = action.reshape(m, 2), old_log_prob.reshape(m, 2).sum(1, keepdim=True)
    adv, v_target = adv.reshape(m, 1), v_target.reshape(m, 1)
    params = ag.trainable()
    mb = min(ag.mini_batch, m)
    for ep in range(ag.mini_epoch):
        perm = perms[ep]
        for i in range(0, m, mb):
            ri = perm[i:i + mb]
            st = {k: v[ri] for k, v in flat.items()}
            mean = torch.clamp(ag.actor(st), -1, 1)
            lp = P.gaussian_log_prob(mean, ag.log_std.expand_as(mean), action[ri]).sum(1, keepdim=True)
            ratio = (lp - old_lp[ri]).exp()
            a = adv[ri]
            actor_loss = -torch.min(ratio * a, torch.clamp(ratio, 1 - ag.clip, 1 + ag.clip) * a).mean()
            critic_loss = F.mse_loss(ag.critic(st), v_target[ri])
            ag.actor_opt.zero_grad(set_to_none=True)
            ag.critic_opt.zero_grad(set_to_none=True)
            (actor_loss + critic_loss).backward()
            ag.allreduce_bytes += D.allreduce_gradients(params)
            ag.actor_opt.step()
            ag.critic_opt.step()
        A._soft_update(ag.critic_target, ag.critic, ag.tau)
    return float(actor_loss.detach()), float(critic_loss.detach())
