"""What the no-gradient critic forwards of an update cost on one GPU, the torch modules against agent_glue.DeviceCritics, in the same run:

  SAC   `critic_target1(nst, na)`, `critic_target2(nst, na)` -- eager (about a hundred launches each) and as one captured graph of the
        same kernels -- against the two-slot call of DeviceCritics (one launch, k_critic_forward on a grid of tiles x 2);
  PPO   the three forwards of BatchedPPO.advantages -- `critic(flat)`, `critic(last_obs)`, `critic_target(flat)`, eager -- against
        DeviceCritics' two calls (critic and target on the block, the critic on last_obs: B / 16 rows, horizon 16).

    python tools/critic_forward_bench.py --out profiles/critic_forward_bench.json

At B = 32 (SAC's default batch: launch count only), 8 192 and 65 536 rows, without the image token (the critics' image encoders stay in
torch on both sides).  Every path is warmed up at every shape; then --reps (default 10) repetitions, in each of which every path is
timed in turn (alternating, so that a drift of the machine touches all of them) over a window of several back-to-back calls between
two device events; the smallest, the median and the largest per-call time of the repetitions are recorded in microseconds, with the
largest difference between the device path's values and the eager ones.  Needs a GPU: there is no fall-back."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hope_amd import ParkingBatch  # noqa: E402
from hope_amd import agent_glue as G  # noqa: E402
from hope_amd import agents as A  # noqa: E402


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def compare(paths, reps, calls, warmup=3):
    """paths: {name: fn} -> {name: {'min_us', 'median_us', 'max_us', 'reps', 'calls_per_window'}}, the paths alternating per repetition"""
    for fn in paths.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in paths}
    for _ in range(reps):
        for k, fn in paths.items():
            us[k].append(window(fn, calls))
    return {k: {'min_us': min(v), 'median_us': statistics.median(v), 'max_us': max(v), 'reps': reps, 'calls_per_window': calls} for k, v in us.items()}


def captured(fn):
    """fn's kernels as one captured graph -> (replay, the static result)"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g.replay, out


def obs(n, dev):
    return {'lidar': torch.randn(n, 120, device=dev), 'target': torch.randn(n, 5, device=dev), 'action_mask': (torch.rand(n, 42, device=dev) < 0.6).float()}


def show(row):
    parts = [f"{k} {v['median_us']:.0f} us [{v['min_us']:.0f}, {v['max_us']:.0f}]" for k, v in row.items() if isinstance(v, dict)]
    print(f"{row['what']} B={row['rows']}: " + ', '.join(parts) + f", max |device - eager| {row['max_abs_diff_device_vs_eager']:.2e}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='critic_forward_bench.json')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--sizes', type=int, nargs='+', default=[32, 8192, 65536])
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a HIP device'
    res = {'device': torch.cuda.get_device_name(0), 'rows': []}
    env = ParkingBatch(64, 32)
    dev = env.device
    torch.manual_seed(0)
    sac = A.BatchedSAC(device=dev, use_img=False, state_norm=False)
    ppo = A.BatchedPPO(device=dev, use_img=False, state_norm=False)
    with torch.no_grad():
        for b in args.sizes:
            calls = 20 if b <= 1024 else 10 if b <= 16384 else 3
            # ---- SAC: the two target critics on one (next_obs, next_action)
            nst, na = obs(b, dev), torch.rand(b, 2, device=dev) * 2 - 1
            crit = G.DeviceCritics(env, (sac.critic_target1, sac.critic_target2))
            eager = lambda: (sac.critic_target1(nst, na), sac.critic_target2(nst, na))  # noqa: E731
            replay, _ = captured(eager)
            row = {'what': 'sac_two_targets', 'rows': b}
            row.update(compare({'eager': eager, 'graph': replay, 'device': lambda: crit(nst, na)}, args.reps, calls))
            row['max_abs_diff_device_vs_eager'] = max(float((d - e).abs().max()) for d, e in zip(crit(nst, na), eager()))
            assert crit.packs == [1, 1]
            res['rows'].append(row)
            show(row)
            # ---- PPO: critic and target on the [N T] block, the critic on last_obs
            flat, last = obs(b, dev), obs(max(b // 16, 2), dev)
            crit = G.DeviceCritics(env, (ppo.critic, ppo.critic_target))
            eager = lambda: (ppo.critic(flat), ppo.critic(last), ppo.critic_target(flat))  # noqa: E731
            device = lambda: (*crit(flat), crit(last, which=(0,))[0])  # noqa: E731
            row = {'what': 'ppo_three_forwards', 'rows': b}
            row.update(compare({'eager': eager, 'device': device}, args.reps, calls))
            v, vt, vl = device()
            e = eager()
            row['max_abs_diff_device_vs_eager'] = max(float((v - e[0]).abs().max()), float((vl - e[1]).abs().max()), float((vt - e[2]).abs().max()))
            assert crit.packs == [1, 1]
            res['rows'].append(row)
            show(row)
    env.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
