"""Shared by tests/test_img_encoder_core.py (CPU, host twin) and tests/test_gpu_img_encoder.py (kernels): the nets with their
deterministic weights, the images, the programmed weight sets of the orientation cases, the host twin's wrapper over exact-size
numpy arrays and torch's forward of the encoder in float32 and float64."""
import copy
import ctypes as C

import numpy as np
import torch

import policy_forward_script as PS
from det_weights import det_fill
from hope_amd import _lib as L
from hope_amd import policy as P

FLOOR = PS.FLOOR              # 2^-22: a few float32 ulps of a value of magnitude 1
FACTOR = PS.FACTOR            # e_twin <= FACTOR * max(e_torch, FLOOR * max(1, max|ref|))
ACTS = ('tanh', 'leaky')
BATCHES = (1, 31, 32, 33, 63, 64, 65, 129)        # the 32-image tile edges of the head kernel
words = PS.words


def make_net(act='tanh', kind='actor'):
    """HopeNet of the reference configuration with the image token, the encoder's activation tanh or LeakyReLU, weights from det_fill"""
    cfg = (P.actor_configs if kind == 'actor' else P.critic_configs)(use_img=True)
    torch.manual_seed(7)
    return det_fill(P.HopeNet(cfg, img_use_tanh=act == 'tanh'), salt=0.25 if act == 'tanh' else 0.6).eval()


def images(b, seed=0):
    """uint8 [b, 3, 64, 64]: image 0 all 0, image 1 all 255, image 2 zero but 255 at the four corners and at one mid-edge pixel per
    side, image 3 a 1-pixel checkerboard; then, alternating, seeded rectangles on a flat ground (what a bird's-eye image looks
    like) and uniform noise"""
    rng = np.random.default_rng(7919 * seed + 13)
    img = np.zeros((b, 3, 64, 64), np.uint8)
    for i in range(b):
        if i == 0:
            continue
        if i == 1:
            img[i] = 255
        elif i == 2:
            for y, x in ((0, 0), (0, 63), (63, 0), (63, 63), (0, 31), (63, 32), (31, 0), (32, 63)):
                img[i, :, y, x] = 255
        elif i == 3:
            yy, xx = np.mgrid[0:64, 0:64]
            img[i] = (((yy + xx) & 1) * 255).astype(np.uint8)
        elif i % 2 == 0:
            img[i] = rng.integers(0, 256, (3, 1, 1), dtype=np.uint8)
            for _ in range(int(rng.integers(2, 9))):
                y0, x0 = rng.integers(0, 60, 2)
                h, w = rng.integers(2, 24, 2)
                img[i, :, y0:y0 + h, x0:x0 + w] = rng.integers(0, 256, (3, 1, 1), dtype=np.uint8)
        else:
            img[i] = rng.integers(0, 256, (3, 64, 64), dtype=np.uint8)
    return img


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def host_params(net):
    """-> (ImgEncParams over numpy copies of the 14 encoder tensors, the arrays: keep them)"""
    sd = {k: np.ascontiguousarray(v.detach().cpu().numpy(), dtype=np.float32) for k, v in net.named_parameters()}
    p, keep = L.ImgEncParams(), []
    for field, key, shape in L.IMGENC_FIELDS:
        assert sd[key].shape == shape, (key, sd[key].shape)
        keep.append(sd[key])
        setattr(p, field, sd[key].ctypes.data)
    return p, keep


def twin(net, img, params=None):
    """hope_imgenc_forward_host over exact-size arrays -> (token [b, 128], features [b, 2048]), both pre-filled with 7"""
    p, keep = params if params is not None else host_params(net)
    img = np.ascontiguousarray(img, dtype=np.uint8)
    b = len(img)
    token, feat = np.full((b, 128), 7.0, np.float32), np.full((b, 2048), 7.0, np.float32)
    L.check(L.load_library().hope_imgenc_forward_host(C.byref(p), L.imgenc_shape(net), _p(img), b, _p(token), _p(feat)), 'hope_imgenc_forward_host')
    return token, feat


def torch_forward(net, img, dtype=torch.float32):
    """the module's own encoder on the CPU in `dtype` -> (token, features) as numpy arrays"""
    m = copy.deepcopy(net).to(dtype)
    with torch.no_grad():
        x = torch.from_numpy(np.ascontiguousarray(img)).to(dtype) * (1.0 / 255.0)
        feat = m.embed_img.net[:3](x)
        token = m.re_embed_img(m.embed_img(x))
    return token.numpy(), feat.numpy()


_REF = {}


def reference(act, b, seed=0):
    """computed once per (act, b, seed) and shared: (net, images, (token64, feat64), (token32, feat32)); treat as read-only"""
    key = (act, b, seed)
    if key not in _REF:
        net, img = make_net(act), images(b, seed)
        _REF[key] = (net, img, torch_forward(net, img, torch.float64), torch_forward(net, img, torch.float32))
    return _REF[key]


def bound(e_torch, ref):
    """the project's accuracy condition with the floor scaled by the output's magnitude: neither output is bounded by 1"""
    return FACTOR * max(e_torch, FLOOR * max(1.0, float(np.abs(ref).max())))


def err(a, ref):
    return float(np.abs(a.astype(np.float64) - ref).max())


def pool_winners(net, img):
    """per block, the set of window positions (dy, dx) that win torch's max pool somewhere (max_pool2d(return_indices=True))"""
    out = []
    with torch.no_grad():
        x = torch.from_numpy(img).to(torch.float32) * (1.0 / 255.0)
        for blk in (net.embed_img.net[0], net.embed_img.net[1]):
            a = blk.layer[1](blk.layer[0](x))
            _, idx = torch.nn.functional.max_pool2d(a, 2, return_indices=True)
            w = a.shape[-1]
            out.append({(int(dy), int(dx)) for dy, dx in zip(((idx // w) % 2).flatten().tolist(), ((idx % w) % 2).flatten().tolist())})
            x = blk(x)
    return out


# ---- the orientation cases: programmed weights, one bright pixel ----
def _blank(act):
    """a net whose convolution and shortcut tensors (weights and biases) are all zero; fc1 and behind stay dense"""
    net = make_net(act)
    with torch.no_grad():
        for blk in (net.embed_img.net[0], net.embed_img.net[1]):
            for t in (blk.layer[0].weight, blk.layer[0].bias, blk.shortcut[0].weight, blk.shortcut[0].bias):
                t.zero_()
    return net


def _carry(net, block):
    """the 1x1 shortcut of `block` (0 or 1) passes its input channels on (channel c -> channel c; block 0's fourth output takes half of
    channel 0), so that the block under test is seen through, or fed by, an average pool and nothing else"""
    w = net.embed_img.net[block].shortcut[0].weight
    with torch.no_grad():
        for c in range(w.shape[1]):
            w[c, c, 0, 0] = 1.0
        if block == 0:
            w[3, 0, 0, 0] = 0.5


def orientation_cases(act='tanh'):
    """-> [(name, net)]: nine nets with ONE nonzero 3x3 tap (co, ci, ky, kx) in block 1 and nine in block 2, every (ky, kx) once per
    block; all other 3x3 weights, all biases of the two blocks and the tested block's shortcut are zero.  The OTHER block's 3x3
    weights are zero too and its shortcut passes the channels on, or nothing would reach the features."""
    cases = []
    for block in (0, 1):
        for t in range(9):
            ky, kx = divmod(t, 3)
            co, ci = (t % 4, t % 3) if block == 0 else ((3 * t + 1) % 8, t % 4)
            net = _blank(act)
            _carry(net, 1 - block)
            with torch.no_grad():
                net.embed_img.net[block].layer[0].weight[co, ci, ky, kx] = 0.75
            cases.append((f'block{block + 1} tap co{co} ci{ci} ky{ky} kx{kx}', net))
    return cases


def shortcut_cases(act='tanh'):
    """one nonzero 1x1 weight (co, ci) per block, seen through / fed by the other block's pass-through shortcut"""
    cases = []
    for block, co, ci in ((0, 2, 1), (0, 3, 2), (1, 5, 3), (1, 6, 0)):
        net = _blank(act)
        _carry(net, 1 - block)
        with torch.no_grad():
            net.embed_img.net[block].shortcut[0].weight[co, ci, 0, 0] = -0.625
        cases.append((f'block{block + 1} shortcut co{co} ci{ci}', net))
    return cases


def fc1_cases(act='tanh'):
    """fc1 with one nonzero column k (and a zero bias), the convolution stack dense"""
    cases = []
    for k in (0, 255, 256, 2047):
        net = make_net(act)
        with torch.no_grad():
            col = net.embed_img.net[3].weight[:, k].clone()
            net.embed_img.net[3].weight.zero_()
            net.embed_img.net[3].bias.zero_()
            net.embed_img.net[3].weight[:, k] = 8.0 * col + 0.25
        cases.append((f'fc1 column {k}', net))
    return cases


def probe_images():
    """uint8 [4, 3, 64, 64]: each image is ONE bright pixel away from the border (255 / 170 / 85 in the three channels, so a channel
    mix-up changes the value), at (y, x) = (20, 36), (25, 41), (34, 30), (43, 19): the four residues modulo 4 in both directions, so a
    one-pixel shift of a tap moves at least one of them into another cell of the twice-pooled grid"""
    img = np.zeros((4, 3, 64, 64), np.uint8)
    for i, (y, x) in enumerate(((20, 36), (25, 41), (34, 30), (43, 19))):
        img[i, :, y, x] = (255, 170, 85)
    return img
