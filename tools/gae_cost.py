"""What PPO's advantage block costs after the critic forwards, at --scenes x --horizon float32 on one GPU: the torch path against the
library's three kernels, in the same run.

    python tools/gae_cost.py --scenes 65536 --horizon 16 --out profiles/gae_cost.json

  torch    what BatchedPPO.advantages does with gae=None once value, v_last and the target critic's values exist: the shifted
           next_value, agent_glue.batched_gae (a Python loop along the horizon), adv + value_target, agents._global_mean_std and
           (adv - m) / (s + 1e-5)
  device   ParkingBatch.gae(..., normalize=True): k_gae_scan, k_gae_merge, k_adv_apply
Both read the same five device tensors.  HIP events around single calls, --warmup calls of each first, then --reps alternating
calls; the median and the spread of each are recorded, with the launches per call: for torch the aten operations that do work
on the device (every dispatched operation but views: each is a kernel or a copy), for the device block its three kernels.
Criterion recorded: the device block is not slower than the torch block.  Needs a GPU: there is no fall-back."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hope_amd import ParkingBatch  # noqa: E402
from hope_amd import agent_glue as G  # noqa: E402
from hope_amd.agents import _global_mean_std  # noqa: E402


VIEWS = ('view', 'select', 'slice', 'unsqueeze', 'squeeze', 'alias', 'expand', 'detach', 'lift_fresh', 't', 'transpose', 'as_strided')


def launches(fn):
    """how many aten operations of one call do work on the device (everything dispatched but views): each is a kernel or a copy"""
    from torch.utils._python_dispatch import TorchDispatchMode

    class Count(TorchDispatchMode):
        n = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if func.overloadpacket.__name__.lstrip('_') not in VIEWS:
                Count.n += 1
            return func(*args, **(kwargs or {}))
    with Count():
        fn()
    return Count.n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenes', type=int, default=65536)
    ap.add_argument('--horizon', type=int, default=16)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--gamma', type=float, default=0.98)
    ap.add_argument('--lam', type=float, default=0.95)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('gae_cost.py measures on a GPU; none is visible')
    n, t = args.scenes, args.horizon
    env = ParkingBatch(n, 32)
    env.enable_gae()
    g = torch.Generator(device='cuda').manual_seed(0)
    reward, value, value_target = (torch.randn((n, t), device='cuda', generator=g) for _ in range(3))
    v_last = torch.randn(n, device='cuda', generator=g)
    done = (torch.rand((n, t), device='cuda', generator=g) < 0.05).float()

    @torch.no_grad()
    def torch_block():
        next_value = torch.cat([value[:, 1:], v_last.unsqueeze(1)], dim=1)
        adv, _ = G.batched_gae(reward, value, next_value, done, args.gamma, args.lam)
        v_target = adv + value_target
        m, s = _global_mean_std(adv)
        return (adv - m) / (s + 1e-5), v_target

    def device_block():
        adv, v_target, _ = env.gae(reward, done, value, v_last, value_target, args.gamma, args.lam)
        return adv, v_target

    blocks = {'torch': torch_block, 'device': device_block}
    for _ in range(args.warmup):
        for fn in blocks.values():
            fn()
    torch.cuda.synchronize()
    a_t, v_t = torch_block()
    a_d, v_d = device_block()
    agree = {'v_target_equal': bool(torch.equal(v_t, v_d)), 'adv_max_abs_diff': float((a_t - a_d).abs().max())}
    ms = {k: [] for k in blocks}
    for _ in range(args.reps):
        for k, fn in blocks.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    res = {'scenes': n, 'horizon': t, 'warmup': args.warmup, 'reps': args.reps, 'gpu': torch.cuda.get_device_name(0), 'agreement': agree}
    for k in blocks:
        a = np.array(ms[k])
        res[k] = {'median_ms': float(np.median(a)), 'min_ms': float(a.min()), 'max_ms': float(a.max()), 'launches': launches(blocks[k]) if k == 'torch' else 3}
    res['criterion_met'] = res['device']['median_ms'] <= res['torch']['median_ms']
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    env.close()


if __name__ == '__main__':
    main()
