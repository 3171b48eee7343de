"""What the planner costs inside a deferred step loop, and k_plan alone, at --scenes scenes on one GPU.

    python tools/planner_cost.py --scenes 65536 --steps 200 --out profiles/planner_cost.json

The loop is the rollout's hot path without the learner: StandInPolicy forward on the observation -> clamp -> the planner's override
-> ParkingBatch.step(auto_reset, defer_rs).  Three variants, three alternating passes of --steps steps each, wall-clock ms per step
(the host synchronisations of the torch planner are part of what is measured, so HIP events around the pass would not do):
  none     no planner
  torch    agent_glue.BatchedRsPlanner as HopeRollout._plan drives it: wait_rs(step), reset(done), set_paths, get_actions, where
  device   ParkingBatch.planner_step(step=last_step(), actions=a): one k_plan launch
k_plan alone: HIP events around --reps back-to-back launches on the state the last device pass left, and around single launches."""
import argparse
import json
import time

import numpy as np
import torch

from hope_amd import ParkingBatch
from hope_amd.agent_glue import BatchedRsPlanner
from hope_amd.rollout import StandInPolicy
from hope_amd.scene_gen import mixed_arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenes', type=int, default=65536)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
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

    envs = {'none': make_env(), 'torch': make_env(), 'device': make_env()}
    envs['device'].enable_planner()
    torch_planner = BatchedRsPlanner(n, device='cuda')
    gens = {k: torch.Generator(device='cuda').manual_seed(1) for k in envs}

    @torch.no_grad()
    def run(mode, steps):
        env, g = envs[mode], gens[mode]
        for _ in range(steps):
            mean, std = policy(env.lidar, env.target, env.action_mask)
            a = torch.clamp(mean + std * torch.randn(mean.shape, device='cuda', generator=g), -1, 1)
            if mode == 'torch':
                env.wait_rs(step=env.last_step())
                torch_planner.reset(env.done.bool())
                torch_planner.set_paths(env.rs_word, env.rs_lengths)
                planned, ex = torch_planner.get_actions()
                a = torch.where(ex.unsqueeze(1), planned.to(a.dtype), a)
            elif mode == 'device':
                env.planner_step(step=env.last_step(), actions=a)
            env.step(a, auto_reset=True, defer_rs=True)

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

    a = torch.zeros((n, 2), dtype=torch.float32, device='cuda')
    env.wait_rs()
    torch.cuda.synchronize()
    busy = float(((env.planner_state()[5] >> np.uint64(13)) & np.uint64(1)).mean())
    launch = lambda: env.planner_step(step=0, actions=a)  # noqa: E731
    for _ in range(20):
        launch()
    back = timed(launch, args.reps)
    single = sorted(timed(launch, 1) for _ in range(50))
    out = {'scenes': n, 'steps_per_pass': args.steps, 'ms_per_step': res,
           'ms_per_step_median': {k: sorted(v)[len(v) // 2] for k, v in res.items()},
           'ms_per_step_spread': {k: round(max(v) - min(v), 4) for k, v in res.items()},
           'k_plan_us_back_to_back': round(back, 2), 'k_plan_us_single_median': round(single[25], 2), 'k_plan_us_single_min': round(single[0], 2),
           'share_of_scenes_replaying_before_k_plan_timing': round(busy, 4),
           'device': torch.cuda.get_device_name(0), 'arch': env.arch}
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')
    for e in envs.values():
        e.close()


if __name__ == '__main__':
    main()
