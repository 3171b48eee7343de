"""What the masked action choice costs inside a deferred step loop, and k_choose alone, at --scenes scenes on one GPU.

    python tools/chooser_cost.py --scenes 65536 --steps 200 --out profiles/chooser_cost.json

The loop is the rollout's action path without the learner: StandInPolicy forward on the observation -> the planner's k_plan
(planner_step(step=last_step())) -> the choice -> ParkingBatch.step(auto_reset, defer_rs).  Two variants of the choice, three
alternating passes of --steps steps each, wall-clock ms per step around a pass that ends in a device synchronise:
  torch    what _AgentCommon.act does: agent_glue.choose_action (mask_action_probs + torch.multinomial), cast, clamp, torch.where
           with the planner's rows, policy.gaussian_log_prob, .to(action dtype).contiguous()
  device   ParkingBatch.choose_actions(mean, log_std, planned=..., executing=...): one k_choose launch, counter-based draws; the
           step takes its action tensor
Criterion recorded: device must not be slower than torch beyond torch's own pass-to-pass spread
(median(device) <= median(torch) + spread(torch)).
k_choose alone: HIP events around --reps back-to-back launches on the last device pass's inputs, and around single launches.
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
from hope_amd.policy import gaussian_log_prob  # noqa: E402
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
        raise SystemExit('chooser_cost.py measures on a GPU; none is visible')
    n = args.scenes
    init = mixed_arrays(2048, levels=('Normal', 'Complex', 'Extrem', 'dlp'), seed=3, max_obst=128)      # both tile classes: the search defers
    sl = np.arange(n) % 2048
    torch.manual_seed(0)
    policy = StandInPolicy().to('cuda').eval()
    log_std = policy.log_std.detach().view(1, 2)

    def make_env():
        env = ParkingBatch(n, 128)
        env.set_scene_arrays(np.arange(n), init[0][sl], init[1][sl], init[2][sl], init[3][sl], init[4][sl])
        env.enable_planner()
        env.reset_obs()
        return env

    envs = {'torch': make_env(), 'device': make_env()}
    envs['device'].enable_chooser()
    gen = torch.Generator(device='cuda').manual_seed(1)
    counter = [0]
    last = {}

    @torch.no_grad()
    def run(mode, steps):
        env = envs[mode]
        for _ in range(steps):
            mean, _ = policy(env.lidar, env.target, env.action_mask)
            planned, ex = env.planner_step(step=env.last_step())
            if mode == 'torch':
                ls = log_std.expand_as(mean)
                a, _ = G.choose_action(mean, ls.exp(), env.action_mask, gen)
                a = torch.clamp(a.to(mean.dtype), -1, 1)
                a = torch.where(ex.unsqueeze(1), planned.to(a.dtype), a)
                last['log_prob'] = gaussian_log_prob(mean, ls, a)
                act = a.to(env.action_dtype).contiguous()
            else:
                act, _, _, last['log_prob'] = env.choose_actions(mean, log_std, None, planned, ex, None, 1, counter[0])
                counter[0] += 1
                last['mean'] = mean
            env.step(act, auto_reset=True, defer_rs=True)

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
    mean = last['mean'].clone()
    mask = env.action_mask.clone()
    planned, ex = env.planned.clone(), env.plan_executing.clone()
    flagged = float((env.chosen_idx >= 64).float().mean())
    launch = lambda: env.choose_actions(mean, log_std, mask, planned, ex, None, 1, 0)  # noqa: E731
    for _ in range(20):
        launch()
    back = timed(launch, args.reps)
    single = sorted(timed(launch, 1) for _ in range(50))
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    spread = {k: round(max(v) - min(v), 4) for k, v in res.items()}
    # bytes k_choose must move per scene: mask row + mean + planned + executing in; action, idx, log_prob out (action_f32 aliases action)
    bytes_per_scene = 42 * mask.element_size() + 2 * mean.element_size() + 16 + 1 + 2 * env.chosen_action.element_size() + 4 + 8
    out = {'scenes': n, 'steps_per_pass': args.steps, 'ms_per_step': res, 'ms_per_step_median': med, 'ms_per_step_spread': spread,
           'criterion': 'median(device) <= median(torch) + spread(torch)', 'criterion_met': bool(med['device'] <= med['torch'] + spread['torch']),
           'k_choose_us_back_to_back': round(back, 2), 'k_choose_us_single_median': round(single[25], 2), 'k_choose_us_single_min': round(single[0], 2),
           'k_choose_bytes_per_scene': bytes_per_scene, 'k_choose_gb_per_s_back_to_back': round(bytes_per_scene * n / (back * 1e-6) / 1e9, 1),
           'share_of_scenes_replaying_in_k_choose_timing': round(float(ex.float().mean()), 4), 'share_of_rows_flagged_in_last_step': round(flagged, 6),
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
