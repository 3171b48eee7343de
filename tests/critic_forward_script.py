"""Shared by tests/test_critic_forward_core.py (CPU, host twin) and tests/test_gpu_critic_forward.py (kernel): the critic nets with
their deterministic weights, the seeded inputs (policy_forward_script's plus the action), the host twin's wrapper over numpy arrays
and the torch forward it is measured against."""
import copy
import ctypes as C

import numpy as np
import torch

import policy_forward_script as PS
from det_weights import det_fill
from hope_amd import _lib as L
from hope_amd import policy as P

# (family, tokens): 'ppo' a critic_configs HopeNet (no action token), 'sac' a SacCritic; the image token with the larger count
KINDS = (('ppo', 3), ('ppo', 4), ('sac', 4), ('sac', 5))
words, bound, _p = PS.words, PS.bound, PS._p


def flags(kind, t):
    """-> (has_img, has_action)"""
    has_action = int(kind == 'sac')
    return t - 3 - has_action, has_action


def make_net(kind, t, salt=0.3):
    """the critic of this kind, weights from det_fill (the image encoder's too)"""
    cfg = P.critic_configs(use_img=bool(flags(kind, t)[0]))
    torch.manual_seed(7)
    net = P.SacCritic(cfg, 2) if kind == 'sac' else P.HopeNet(cfg)
    return det_fill(net, salt=salt).eval()


def inputs(b, kind, t, seed=0, n_nets=1):
    """policy_forward_script.inputs, with 'img_token' [n_nets, b, 128] (or None) and 'action' [b, 2] float32 in [-1, 1], row 0 =
    (1, -1) and row 1 = 0 (or None)"""
    has_img, has_action = flags(kind, t)
    x = PS.inputs(b, 4 if has_img else 3, seed)
    rng = np.random.default_rng(7919 * b + 31 * t + seed)
    x['img_token'] = rng.standard_normal((n_nets, b, 128)).astype(np.float32) if has_img else None
    x['action'] = None
    if has_action:
        a = rng.uniform(-1.0, 1.0, (b, 2)).astype(np.float32)
        a[0] = (1.0, -1.0)
        if b > 1:
            a[1] = 0.0
        x['action'] = a
    return x


def host_params(net):
    """-> (CriticParams over numpy copies of the net's parameters, the arrays: keep them)"""
    has_img, has_action = L.critic_shape(net)
    sd = {k: np.ascontiguousarray(v.detach().cpu().numpy(), dtype=np.float32) for k, v in L.critic_net(net).named_parameters()}
    p, keep = L.CriticParams(), []
    for field, key in L.CRITIC_FIELDS[:len(L.CRITIC_FIELDS) if has_action else len(L.POLICY_FIELDS)]:
        keep.append(sd[key])
        setattr(p, field, sd[key].ctypes.data)
    return p, keep


def twin(net, x, params=None, which=0):
    """hope_critic_forward_host over exact-size arrays, the image token x['img_token'][which] -> out [b] (pre-filled with 7)"""
    has_img, has_action = L.critic_shape(net)
    p, keep = params if params is not None else host_params(net)
    b = len(x['lidar'])
    out = np.full((b,), 7.0, np.float32)
    tok = np.ascontiguousarray(x['img_token'][which]) if has_img else None
    L.check(L.load_library().hope_critic_forward_host(C.byref(p), has_img, has_action, _p(x['lidar']), _p(x['target']), _p(x['mask']), _p(tok),
                                                      _p(x['action']), b, _p(out)), 'hope_critic_forward_host')
    return out


def torch_forward(net, x, dtype=torch.float32, which=0):
    """the module's own forward on the CPU in `dtype`, the image token taken as given -> [b]"""
    m = copy.deepcopy(L.critic_net(net)).to(dtype)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)  # noqa: E731
    with torch.no_grad():
        f = [m.embed_lidar(t(x['lidar'])), m.embed_tgt(t(x['target'])), m.embed_am(t(x['mask']))]
        if x['img_token'] is not None:
            f.append(t(x['img_token'][which]))
        if x['action'] is not None:
            f.append(m.embed_action(t(x['action'])))
        out = m.net(torch.stack(f, dim=1))
    return out.numpy()[:, 0]


def errors(net, x, got):
    """-> (e_torch, e_got): the largest absolute differences of torch's float32 forward and of `got` from the float64 forward"""
    ref = torch_forward(net, x, torch.float64)
    e_torch = float(np.abs(torch_forward(net, x, torch.float32).astype(np.float64) - ref).max())
    return e_torch, float(np.abs(got.astype(np.float64) - ref).max())


def nobs(x, device='cpu'):
    """the inputs as the observation dict (and action) a DeviceCritics takes"""
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    d = {'lidar': t(x['lidar']), 'target': t(x['target']), 'action_mask': t(x['mask'])}
    if x['img_token'] is not None:
        d['img_token'] = t(x['img_token'])
    return d, t(x['action'])
