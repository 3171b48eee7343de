"""What one body of BatchedSAC.update costs on one GPU without the network forwards and backwards -- the sampled actions, the Q target, the
three losses and the backward pass down to the gradients at the networks' outputs -- on the torch path (the elementwise lines, autograd
through them and the requires_grad loop over the critics' parameters) against agent_glue.DeviceSacUpdate (k_sac_sample, k_sac_critic,
k_sac_seed, k_sac_policy, k_sac_merge), in the same run.

    python tools/sac_update_cost.py --out profiles/sac_update_cost.json

The networks' outputs are stand-in leaf tensors, and the two critics at the sampled action are stood in by q_k(a) = c_k + sum_d a_d J_kd
(three launches each, the same in both bodies), so both bodies end in the same gradients: at the two critic outputs, at the actor's
output, at log_std and at log_alpha (their largest difference under the same noise is recorded).  The parameters whose requires_grad
the torch path flips are those of two real SacCritic networks, which are never run.  At B = 32 and B = 4096: 50 warm-up bodies of
each, then five windows of 1000 bodies of each, alternating, a host clock around every window with a device synchronise at both ends;
the windows and their median are recorded in microseconds per body.  Then the launches of one body of each as the profiler sees them
(torch.profiler: every kernel and device copy), in a pass of its own.  Needs a GPU: there is no fall-back."""
import argparse
import json
import math
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

GAMMA, TARGET_ENTROPY = 0.99, -2.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='sac_update_cost.json')
    OUT = ap.parse_args().out
    assert torch.cuda.is_available(), 'needs a HIP device'
    env = ParkingBatch(64, 32)
    dev = env.device
    torch.manual_seed(0)
    blk = G.DeviceSacUpdate(env)
    critics = [P.SacCritic(P.critic_configs(use_img=False), 2).to(dev) for _ in range(2)]
    cparams = [p for c in critics for p in c.parameters()]
    log_std = torch.tensor([[-0.3, 0.2]], device=dev, requires_grad=True)
    log_alpha = torch.tensor(math.log(0.01), dtype=torch.float64, device=dev, requires_grad=True)
    res = {'critic_parameter_tensors': len(cparams)}
    for b in (32, 4096):
        raw_n = 0.7 * torch.randn(b, 2, device=dev)                             # the actor at the next observation
        qt1, qt2 = torch.randn(b, 1, device=dev), torch.randn(b, 1, device=dev)  # the target critics at the sampled next action
        q1 = torch.randn(b, 1, device=dev).requires_grad_()                     # the critics at the stored action
        q2 = torch.randn(b, 1, device=dev).requires_grad_()
        raw = (0.7 * torch.randn(b, 2, device=dev)).requires_grad_()            # the actor at the observation
        reward, done = torch.randn(b, device=dev), (torch.rand(b, device=dev) < 0.2).float()
        c1, c2 = torch.randn(b, 1, device=dev), torch.randn(b, 1, device=dev)
        J1, J2 = torch.randn(b, 2, device=dev), torch.randn(b, 2, device=dev)
        leaves = (q1, q2, raw, log_std, log_alpha)

        def critic_at(a, c, J):
            return c + (a * J).sum(-1, keepdim=True)

        def sample(r):
            mean = torch.clamp(r, -1, 1)
            ls = log_std.expand_as(mean)
            eps = torch.randn_like(mean)
            a = torch.clamp(mean + ls.exp() * eps, -1, 1)
            return a, P.gaussian_log_prob(mean, ls, a)

        def torch_body():
            rw, dn = reward.view(-1, 1), done.view(-1, 1)
            alpha = log_alpha.exp().detach().to(rw.dtype)
            with torch.no_grad():
                na, nlp = sample(raw_n)
                nlp = nlp.sum(-1, keepdim=True)
                q_t = torch.min(qt1, qt2)
                q_target = rw + (1 - dn) * GAMMA * (q_t - alpha * nlp)
            q1_loss = F.mse_loss(q1, q_target)
            q2_loss = F.mse_loss(q2, q_target)
            q1.grad = q2.grad = None
            (q1_loss + q2_loss).backward()
            for p in cparams:
                p.requires_grad_(False)
            a_, lp = sample(raw)
            lp = lp.sum(-1, keepdim=True)
            actor_loss = (alpha * lp - torch.min(critic_at(a_, c1, J1), critic_at(a_, c2, J2))).mean()
            raw.grad = log_std.grad = None
            actor_loss.backward()
            for p in cparams:
                p.requires_grad_(True)
            alpha_loss = (log_alpha.exp() * (-lp - TARGET_ENTROPY).detach()).mean()
            log_alpha.grad = None
            alpha_loss.backward()

        def device_body():
            with torch.no_grad():
                eps = torch.randn_like(raw_n)
                _, nlp = blk.sample(raw_n, log_std, eps)
            _, g_q1, g_q2, _ = blk.critic(q1, q2, qt1, qt2, nlp, reward, done, log_alpha, GAMMA)
            q1.grad = q2.grad = None
            torch.autograd.backward((q1, q2), (g_q1.view(q1.shape), g_q2.view(q2.shape)))
            eps = torch.randn_like(raw)
            a = blk.sample(raw, log_std, eps)[0].detach().requires_grad_()
            p1, p2 = critic_at(a, c1, J1), critic_at(a, c2, J2)
            s1, s2 = blk.seed(p1, p2)
            g_action, = torch.autograd.grad((p1, p2), (a,), (s1.view(p1.shape), s2.view(p2.shape)))
            g_raw, g_log_std, g_log_alpha, _ = blk.policy(raw, log_std, eps, p1, p2, g_action, log_alpha, TARGET_ENTROPY)
            raw.grad = log_std.grad = None
            torch.autograd.backward((raw, log_std), (g_raw, g_log_std.view(log_std.shape)))
            log_alpha.grad = g_log_alpha

        def window(body, iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                body()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / iters * 1e6

        for body in (torch_body, device_body):                     # warm-up: code objects, allocator, the per-B tensors
            window(body, 50)
        grads = []
        for body in (torch_body, device_body):                     # the two paths give the same gradients up to the last bits
            torch.manual_seed(1)
            body()
            torch.cuda.synchronize()
            grads.append([x.grad.detach().double().clone() for x in leaves])
        diff = [float((a - c).abs().max()) for a, c in zip(*grads)]
        iters = 1000
        tt, td = [], []
        for _ in range(5):
            tt.append(window(torch_body, iters))
            td.append(window(device_body, iters))
        res[b] = {'torch_us': tt, 'device_us': td, 'torch_median_us': float(np.median(tt)), 'device_median_us': float(np.median(td)),
                  'max_abs_gradient_difference': dict(zip(('q1', 'q2', 'raw', 'log_std', 'log_alpha'), diff)), 'iterations_per_window': iters}
        print(b, res[b], flush=True)
        with open(OUT, 'w') as f:
            json.dump(res, f, indent=1)
    # launches of one body, counted by the profiler (its own pass, after the timings)
    from torch.profiler import ProfilerActivity, profile
    for name, body in (('torch', torch_body), ('device', device_body)):       # (the bodies of the last size: the count does not depend on it)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            body()
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
