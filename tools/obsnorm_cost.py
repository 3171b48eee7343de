"""What the observation normalisation costs inside a deferred step loop, and its kernels alone, at --scenes scenes on one GPU.

    python tools/obsnorm_cost.py --scenes 65536 --steps 200 --out profiles/obsnorm_cost.json

The loop is the rollout's observation path without the learner: step(auto_reset, defer_rs) -> fold the new observation into the
running statistics -> normalise it -> StandInPolicy forward on the normalised observation -> the clamped mean as the next action.
Two variants of the normalisation, three alternating passes of --steps steps each, wall-clock ms per step around a pass that ends in
a device synchronise:
  torch    obs_norm=None: agent_glue.BatchedStateNorm.update, then .normalize and the three .float() casts of _AgentCommon._norm_obs
  device   obs_norm='device': ParkingBatch.obsnorm() -- k_obsnorm_partial, k_obsnorm_merge, k_obsnorm_apply -- and the mask's cast
Criterion recorded: device must not be slower than torch beyond torch's own pass-to-pass spread
(median(device) <= median(torch) + spread(torch)).
The kernels alone: HIP events around --reps back-to-back calls on the last observation, and around single calls, of the update
(k_obsnorm_partial + k_obsnorm_merge: one entry point launches both, so they are timed as a pair) and of k_obsnorm_apply.
Needs a GPU: there is no fall-back."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hope_amd import ParkingBatch  # noqa: E402
from hope_amd import agent_glue as G  # noqa: E402
from hope_amd.rollout import StandInPolicy  # noqa: E402
from hope_amd.scene_gen import mixed_arrays  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenes', type=int, default=65536)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('obsnorm_cost.py measures on a GPU; none is visible')
    n = args.scenes
    init = mixed_arrays(2048, levels=('Normal', 'Complex', 'Extrem', 'dlp'), seed=3, max_obst=128)      # both tile classes: the search defers
    sl = np.arange(n) % 2048
    torch.manual_seed(0)
    policy = StandInPolicy().to('cuda').eval()

    def make_env():
        env = ParkingBatch(n, 128)
        env.set_scene_arrays(np.arange(n), init[0][sl], init[1][sl], init[2][sl], init[3][sl], init[4][sl])
        env.reset_obs()
        return env

    envs = {'torch': make_env(), 'device': make_env()}
    envs['device'].enable_obsnorm()
    sn = G.BatchedStateNorm(device='cuda')

    @torch.no_grad()
    def run(mode, steps):
        env = envs[mode]
        for _ in range(steps):
            if mode == 'torch':
                raw = {'lidar': env.lidar, 'target': env.target}
                sn.update(raw)
                nz = sn.normalize(raw)
                nl, nt = nz['lidar'].float(), nz['target'].float()
            else:
                nl, nt = env.obsnorm()
            mean, _ = policy(nl, nt, env.action_mask.float())
            env.step(mean.clamp(-1, 1).to(env.action_dtype).contiguous(), auto_reset=True, defer_rs=True)

    def timed_pass(mode):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(mode, args.steps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1000.0 / args.steps

    for mode in envs:
        run(mode, 20)                                                     # warm-up
    res = {k: [] for k in envs}
    for _ in range(args.passes):
        for mode in envs:
            res[mode].append(round(timed_pass(mode), 4))
    env = envs['device']
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn, reps):
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1000.0 / reps                  # us

    env.wait_rs()
    torch.cuda.synchronize()
    lidar, target = env.lidar.clone(), env.target.clone()
    calls = {'update_partial_plus_merge': lambda: env.obsnorm(lidar, target, update=True, normalize=False),
             'k_obsnorm_apply': lambda: env.obsnorm(lidar, target, update=False, normalize=True)}
    kern = {}
    for name, fn in calls.items():
        for _ in range(20):
            fn()
        back = timed(fn, args.reps)
        single = sorted(timed(fn, 1) for _ in range(50))
        kern[name] = {'us_back_to_back': round(back, 2), 'us_single_median': round(single[25], 2), 'us_single_min': round(single[0], 2)}
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    spread = {k: round(max(v) - min(v), 4) for k, v in res.items()}
    # bytes per scene: the update reads the 125 words twice (the second pass out of L2); the apply reads them once and writes 125 float32
    es = lidar.element_size()
    kern['update_partial_plus_merge']['bytes_per_scene_from_memory'] = 125 * es
    kern['k_obsnorm_apply']['bytes_per_scene'] = 125 * es + 125 * 4
    kern['k_obsnorm_apply']['gb_per_s_back_to_back'] = round((125 * es + 125 * 4) * n / (kern['k_obsnorm_apply']['us_back_to_back'] * 1e-6) / 1e9, 1)
    out = {'scenes': n, 'steps_per_pass': args.steps, 'ms_per_step': res, 'ms_per_step_median': med, 'ms_per_step_spread': spread,
           'criterion': 'median(device) <= median(torch) + spread(torch)', 'criterion_met': bool(med['device'] <= med['torch'] + spread['torch']),
           'kernels': kern, 'n_state_at_the_end': env.obsnorm_count(), 'device': torch.cuda.get_device_name(0), 'arch': env.arch}
    print(json.dumps(out))
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')
    for e in envs.values():
        e.close()


if __name__ == '__main__':
    main()
