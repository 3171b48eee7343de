"""Shared by tests/test_policy_forward_core.py (CPU, host twin) and tests/test_gpu_policy_forward.py (kernel): the nets with their
deterministic weights, the seeded inputs, the host twin's wrapper over numpy arrays and the torch forwards it is measured against."""
import copy
import ctypes as C

import numpy as np
import torch

from det_weights import det_fill
from hope_amd import _lib as L
from hope_amd import policy as P

FLOOR = 2.0 ** -22            # a few float32 ulps of an output bounded by 1
FACTOR = 4.0                  # e_twin <= FACTOR * max(e_torch, FLOOR)
KINDS = (('actor', 3), ('actor', 4), ('critic', 3), ('critic', 4))


def make_net(kind, n_tokens):
    """HopeNet of the reference configuration ('actor': 2 outputs behind a tanh; 'critic': 1 linear output), n_tokens 3 (no image)
    or 4, weights from det_fill (the image encoder's too)"""
    cfg = (P.actor_configs if kind == 'actor' else P.critic_configs)(use_img=n_tokens == 4)
    torch.manual_seed(7)
    return det_fill(P.HopeNet(cfg), salt=0.25 if kind == 'actor' else 0.75).eval()


def inputs(b, n_tokens, seed=0):
    """-> {'lidar' [b, 120], 'target' [b, 5], 'mask' [b, 42], 'img_token' [b, 128] or None}, float32: lidar and target roughly unit
    normal with a few entries at +-10, the mask in {0, 1} with row 0 (and every 17th) all zero and row 1 all one"""
    rng = np.random.default_rng(1000003 * b + 17 * n_tokens + seed)
    lidar = rng.standard_normal((b, L.LIDAR_NUM)).astype(np.float32)
    target = rng.standard_normal((b, L.TARGET_DIM)).astype(np.float32)
    for a in (lidar, target):
        flat = a.reshape(-1)
        at = rng.choice(flat.size, size=max(2, flat.size // 97), replace=False)
        flat[at] = np.where(np.arange(len(at)) % 2 == 0, 10.0, -10.0).astype(np.float32)
    mask = (rng.random((b, L.N_ACTION)) < 0.6).astype(np.float32)
    mask[::17] = 0.0
    if b > 1:
        mask[1] = 1.0
    token = rng.standard_normal((b, 128)).astype(np.float32) if n_tokens == 4 else None
    return {'lidar': lidar, 'target': target, 'mask': mask, 'img_token': token}


def words(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def host_params(net):
    """-> (PolicyParams over numpy copies of the net's parameters, the arrays: keep them)"""
    sd = {k: np.ascontiguousarray(v.detach().cpu().numpy(), dtype=np.float32) for k, v in net.named_parameters()}
    p, keep = L.PolicyParams(), []
    for field, key in L.POLICY_FIELDS:
        keep.append(sd[key])
        setattr(p, field, sd[key].ctypes.data)
    return p, keep


def shape_of(net):
    return L.policy_shape(net)


def twin(net, x, params=None):
    """hope_policy_forward_host over exact-size arrays -> out [b, out_dim] (pre-filled with 7)"""
    n_tokens, out_dim, tanh_out = shape_of(net)
    p, keep = params if params is not None else host_params(net)
    b = len(x['lidar'])
    out = np.full((b, out_dim), 7.0, np.float32)
    L.check(L.load_library().hope_policy_forward_host(C.byref(p), n_tokens, out_dim, tanh_out, _p(x['lidar']), _p(x['target']), _p(x['mask']),
                                                      _p(x['img_token']), b, _p(out)), 'hope_policy_forward_host')
    return out


def torch_forward(net, x, dtype=torch.float32):
    """the module's own forward on the CPU in `dtype` (float64: net.double() on float64 inputs), the image token taken as given"""
    m = copy.deepcopy(net).to(dtype)
    t = lambda k: torch.from_numpy(x[k]).to(dtype)  # noqa: E731
    with torch.no_grad():
        f = [m.embed_lidar(t('lidar')), m.embed_tgt(t('target')), m.embed_am(t('mask'))]
        if x['img_token'] is not None:
            f.append(t('img_token'))
        out = m.net(torch.stack(f, dim=1))
        out = torch.tanh(out) if m.tanh_out else out
    return out.numpy()


def errors(net, x, got):
    """-> (e_torch, e_got): the largest absolute differences of torch's float32 forward and of `got` from the float64 forward"""
    ref = torch_forward(net, x, torch.float64)
    e_torch = float(np.abs(torch_forward(net, x, torch.float32).astype(np.float64) - ref).max())
    return e_torch, float(np.abs(got.astype(np.float64) - ref).max())


def bound(e_torch):
    return FACTOR * max(e_torch, FLOOR)
