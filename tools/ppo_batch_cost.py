"""What one body of BatchedPPO.update's inner loop costs on one GPU without the two network forwards -- the gather of the minibatch, the
loss and the backward pass down to the gradients at the networks' outputs -- on the torch path (index gathers, the elementwise loss,
autograd through it) against agent_glue.DevicePpoBatch (k_ppo_gather, k_ppo_loss, k_ppo_merge), in the same run.

    python tools/ppo_batch_cost.py --out profiles/ppo_batch_cost.json

A full ring of 4096 x 4 transitions; the networks' outputs are stand-in leaf tensors, so both bodies end in the same three gradients
(their largest difference is recorded).  At mb = 32 and mb = 4096: 50 warm-up bodies of each, then five windows of 1500 bodies of each,
alternating, a host clock around every window with a device synchronise at both ends; the windows and their median are recorded in
microseconds per body.  Then the launches of one body of each as the profiler sees them (torch.profiler: every kernel and device
copy), in a pass of its own.  Needs a GPU: there is no fall-back."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hope_amd import ParkingBatch  # noqa: E402
from hope_amd import agent_glue as G  # noqa: E402
from hope_amd import policy as P  # noqa: E402
from hope_amd.rollout import DeviceTransitionRing  # noqa: E402

N, T, CLIP = 4096, 4, 0.2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='ppo_batch_cost.json')
    OUT = ap.parse_args().out
    assert torch.cuda.is_available(), 'needs a HIP device'
    env = ParkingBatch(N, 32)
    dev = env.device
    torch.manual_seed(0)
    ring = DeviceTransitionRing(env, T, ('lidar', 'target', 'action_mask'))
    for v in ring.obs.values():
        v.copy_(torch.randn(v.shape, device=dev))
    ring.action.copy_(torch.randn(N, T, 2, device=dev).clamp(-1, 1))
    ring.log_prob.copy_(-1.0 + 0.3 * torch.randn(N, T, 2, device=dev))
    ring.head, ring.size = 0, T
    m = N * T
    adv, v_target = torch.randn(N, T, device=dev), torch.randn(N, T, device=dev)
    log_std = torch.zeros(1, 2, device=dev, requires_grad=True)
    mbatch = G.DevicePpoBatch(env, ring)
    res = {}
    for mb in (32, 4096):
        perm = torch.randperm(m, device=dev)
        raw = (0.7 * torch.randn(mb, 2, device=dev)).requires_grad_()
        value = torch.randn(mb, 1, device=dev).requires_grad_()
        flat = {k: v.reshape((m,) + v.shape[2:]) for k, v in ring.obs.items()}
        action, old_lp = ring.action.reshape(m, 2), ring.log_prob.reshape(m, 2).sum(1, keepdim=True)
        a_, vt_ = adv.reshape(m, 1), v_target.reshape(m, 1)

        def torch_body(i):
            ri = perm[i:i + mb]
            st = {k: v[ri] for k, v in flat.items()}
            mean = torch.clamp(raw, -1, 1)
            lp = P.gaussian_log_prob(mean, log_std.expand_as(mean), action[ri]).sum(1, keepdim=True)
            ratio = (lp - old_lp[ri]).exp()
            a = a_[ri]
            actor_loss = -torch.min(ratio * a, torch.clamp(ratio, 1 - CLIP, 1 + CLIP) * a).mean()
            critic_loss = F.mse_loss(value, vt_[ri])
            raw.grad = value.grad = log_std.grad = None
            (actor_loss + critic_loss).backward()
            return st

        def device_body(i):
            ri = perm[i:i + mb]
            st, batch = mbatch.gather(adv, v_target, ri)
            raw.grad = value.grad = log_std.grad = None
            mbatch.backward(raw, value, log_std, batch, CLIP)
            return st

        def window(body, iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(iters):
                body((k * mb) % (m - mb + 1))
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / iters * 1e6

        for body in (torch_body, device_body):                     # warm-up: code objects, allocator, the per-mb tensors
            window(body, 50)
        # the two paths give the same seeds up to the last bits
        torch_body(0); g_t = [raw.grad.clone(), value.grad.clone(), log_std.grad.clone()]
        device_body(0); g_d = [raw.grad.clone(), value.grad.clone(), log_std.grad.clone()]
        diff = [float((a - b).abs().max()) for a, b in zip(g_t, g_d)]
        iters = 1500
        tt, td = [], []
        for _ in range(5):
            tt.append(window(torch_body, iters))
            td.append(window(device_body, iters))
        res[mb] = {'torch_us': tt, 'device_us': td, 'torch_median_us': float(np.median(tt)), 'device_median_us': float(np.median(td)),
                   'max_abs_seed_difference': diff, 'iterations_per_window': iters}
        print(mb, res[mb], flush=True)
        with open(OUT, 'w') as f:
            json.dump(res, f, indent=1)
    # launches of one body, counted by the profiler (its own pass, after the timings)
    from torch.profiler import ProfilerActivity, profile
    for name, body in (('torch', torch_body), ('device', device_body)):       # (the bodies of the last size: the count does not depend on it)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            body(0)
            torch.cuda.synchronize()
        kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        res['launches_' + name] = len(kernels)
        res['kernels_' + name] = sorted({e.name[:60] for e in kernels})
        print(name, 'device events of one body:', len(kernels), flush=True)
        with open(OUT, 'w') as f:
            json.dump(res, f, indent=1)
    env.close()


if __name__ == '__main__':
    main()
