"""What the transition ring costs between the env step and the policy on one GPU: rollout.TransitionRing (torch copies, sums and
gathers) against rollout.DeviceTransitionRing (the library's four kernels), in the same run.

    python tools/ring_cost.py --out profiles/ring_cost.json

  push     one step at --scenes x --horizon: write_before, write_after and the tally of episodes, successes and rewards
             torch    TransitionRing.write_before / write_after and HopeRollout.collect_step's three tallies
             device   DeviceTransitionRing.write_before / write_after(reward, done, status): k_ring_before, k_ring_after, k_ring_tally
  sample   one sample(--batch) from a full ring at --scenes x --sample-horizon
             torch    TransitionRing.sample (two randint, the index arithmetic, a gather per key for obs and next_obs, a where per key)
             device   DeviceTransitionRing.sample: k_ring_sample
Both rings hold the same contents and read the same step outputs.  HIP events around single calls, --warmup calls of each first, then
--reps alternating calls; the median and the spread of each are recorded, with the launches of one call as the profiler sees them
(torch.profiler: every kernel and device copy).  Criterion recorded: neither device block is slower than its torch block.  Needs a
GPU: there is no fall-back."""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hope_amd import ParkingBatch  # noqa: E402
from hope_amd.rollout import DeviceTransitionRing, TransitionRing  # noqa: E402

KEYS = ('lidar', 'target', 'action_mask')


def launches(fn):
    """the kernels and device copies of one call, from the profiler"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(e.device_type).endswith('CUDA')]
    return len(names), sorted({short_name(x) for x in names})


def short_name(kernel):
    """a kernel's name without its return type, template arguments and parameters"""
    import re
    name = re.sub(r'^void\s+', '', kernel).replace('(anonymous namespace)::', '')
    return re.split(r'[<(]', name, maxsplit=1)[0].strip()


def measure(blocks, warmup, reps):
    for _ in range(warmup):
        for fn in blocks.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in blocks}
    for _ in range(reps):
        for k, fn in blocks.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    out = {}
    for k, fn in blocks.items():
        a = np.array(ms[k])
        count, names = launches(fn)
        out[k] = {'median_ms': float(np.median(a)), 'min_ms': float(a.min()), 'max_ms': float(a.max()), 'launches': count, 'kernels': names}
    out['criterion_met'] = out['device']['median_ms'] <= out['torch']['median_ms']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenes', type=int, default=65536)
    ap.add_argument('--horizon', type=int, default=16)
    ap.add_argument('--sample-horizon', type=int, default=8)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ring_cost.py measures on a GPU; none is visible')
    n = args.scenes
    env = ParkingBatch(n, 32)
    dev = env.device
    g = torch.Generator(device=dev).manual_seed(0)
    nobs = {'lidar': torch.randn((n, 120), device=dev, generator=g), 'target': torch.randn((n, 5), device=dev, generator=g),
            'action_mask': (torch.rand((n, 42), device=dev, generator=g) < 0.7).float()}
    action, log_prob = torch.randn((n, 2), device=dev, generator=g), torch.randn((n, 2), device=dev, generator=g)
    step = types.SimpleNamespace(reward=torch.randn(n, device=dev, generator=g).to(env.obs_dtype),
                                 done=(torch.rand(n, device=dev, generator=g) < 0.05).to(torch.uint8),
                                 status=torch.randint(0, 6, (n,), device=dev, generator=g).to(torch.int32))
    res = {'scenes': n, 'warmup': args.warmup, 'reps': args.reps, 'gpu': torch.cuda.get_device_name(0)}

    # ---- push and tally of one step ----
    t_ring, d_ring = TransitionRing(n, args.horizon, KEYS, dev), DeviceTransitionRing(env, args.horizon, KEYS)
    tally = types.SimpleNamespace(episodes=torch.zeros((), dtype=torch.int64, device=dev), successes=torch.zeros((), dtype=torch.int64, device=dev),
                                  reward_sum=torch.zeros((), dtype=torch.float64, device=dev))

    @torch.no_grad()
    def torch_push():                                 # HopeRollout.collect_step with ring=None, the ring's share
        t_ring.write_before(nobs, action, log_prob)
        t_ring.write_after(step.reward, step.done)
        done = step.done.bool()
        tally.episodes += done.sum()
        tally.successes += (step.status == 2).sum()
        tally.reward_sum += step.reward.sum(dtype=torch.float64)

    @torch.no_grad()
    def device_push():
        d_ring.write_before(nobs, action, log_prob)
        d_ring.write_after(step.reward, step.done, step.status)

    res['push'] = dict(horizon=args.horizon, **measure({'torch': torch_push, 'device': device_push}, args.warmup, args.reps))
    torch.cuda.synchronize()
    same = all(torch.equal(t_ring.obs[k], d_ring.obs[k]) for k in KEYS) and torch.equal(t_ring.reward, d_ring.reward) and torch.equal(t_ring.done, d_ring.done)
    res['push']['agreement'] = {'ring_equal': bool(same), 'episodes_equal': int(tally.episodes) == int(d_ring.counts[0]),
                                'reward_sum_rel_diff': abs(float(tally.reward_sum) - float(d_ring.reward_sum)) / max(abs(float(tally.reward_sum)), 1e-300)}

    # ---- one batch from a full ring ----
    del t_ring, d_ring
    T = args.sample_horizon
    t_ring, d_ring = TransitionRing(n, T, KEYS, dev), DeviceTransitionRing(env, T, KEYS)
    for _ in range(T + 3):
        for r in (t_ring, d_ring):
            r.write_before(nobs, action, log_prob)
            r.write_after(step.reward, step.done)
    gen = torch.Generator(device=dev).manual_seed(1)

    @torch.no_grad()
    def torch_sample():
        return t_ring.sample(args.batch, nobs, gen)

    @torch.no_grad()
    def device_sample():
        return d_ring.sample(args.batch, nobs)

    res['sample'] = dict(horizon=T, batch=args.batch, **measure({'torch': torch_sample, 'device': device_sample}, args.warmup, args.reps))
    b = device_sample()
    s, j = b['idx'][:, 0].long(), (b['idx'][:, 1].long() - (d_ring.head - d_ring.size)) % T
    ref = t_ring.sample(args.batch, nobs, index=(s, j))
    res['sample']['agreement'] = {'batch_equal': bool(all(torch.equal(b['obs'][k], ref['obs'][k]) and torch.equal(b['next_obs'][k], ref['next_obs'][k]) for k in KEYS)
                                                      and torch.equal(b['reward'], ref['reward']))}
    res['criterion_met'] = res['push']['criterion_met'] and res['sample']['criterion_met']
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    env.close()


if __name__ == '__main__':
    main()
