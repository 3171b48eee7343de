"""What the evaluator's bookkeeping costs inside its step loop, and the tracker's kernels alone, at --scenes scenes on one GPU.

    python tools/evaltrack_cost.py --scenes 65536 --steps 200 --out profiles/evaltrack_cost.json

The loop is BatchedEvaluator.run itself (BatchedPPO, post_proc_action) with the device planner, chooser and observation norm in both
variants, so that only the bookkeeping differs; every pass restarts all episodes on the same maps and runs --steps steps (a multiple
of poll_every).  Two variants, three alternating passes each, wall-clock ms per env step around a pass that ends in a device
synchronise:
  torch    tracker=None: the torch one-liners and `bool(alive.any())`, a host synchronisation, every step
  device   tracker='device', poll_every=8: k_eval_override before and k_eval_track after the env step, the host asks every 8 steps
Criterion recorded: device must not be slower than torch beyond torch's own pass-to-pass spread
(median(device) <= median(torch) + spread(torch)).
The kernels alone: HIP events around --reps back-to-back calls on the env's last outputs, and around single calls, of k_eval_begin,
k_eval_override (every scene stuck: the most it writes) and k_eval_track.
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
from hope_amd import agents as A  # noqa: E402
from hope_amd import evaluate as E  # noqa: E402
from hope_amd.scene_gen import mixed_arrays  # noqa: E402

POLL_EVERY = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenes', type=int, default=65536)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('evaltrack_cost.py measures on a GPU; none is visible')
    n = args.scenes
    init = mixed_arrays(2048, levels=('Normal', 'Complex', 'Extrem', 'dlp'), seed=3, max_obst=128)
    sl = np.arange(n) % 2048
    everyone = torch.ones(n, dtype=torch.uint8, device='cuda')

    def make(tracker):
        torch.manual_seed(0)
        agent = A.BatchedPPO(device='cuda', use_img=False)                # one per variant: obs_norm='device' binds its norm to the env
        env = ParkingBatch(n, 128)
        env.set_scene_arrays(np.arange(n), init[0][sl], init[1][sl], init[2][sl], init[3][sl], init[4][sl])
        ev = E.BatchedEvaluator(env, agent, post_proc_action=True, use_planner='device', chooser='device', obs_norm='device', seed=5,
                                tracker=tracker, poll_every=POLL_EVERY)
        calls = [0]
        orig = env.step

        def counted(actions, **kw):
            calls[0] += 1
            return orig(actions, **kw)
        env.step = counted
        return env, ev, calls

    runs = {'torch': make(None), 'device': make('device')}
    finished = {}

    def timed_pass(mode, steps):
        env, ev, calls = runs[mode]
        env.restart(everyone)
        calls[0] = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rec = ev.run(max_steps=steps, gather=False)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1000.0
        finished[mode] = int((rec[:, 0] != 1).sum())
        return dt / max(calls[0], 1), calls[0]

    for mode in runs:
        timed_pass(mode, 16)                                              # warm-up
    res = {k: [] for k in runs}
    steps_taken = {k: [] for k in runs}
    for _ in range(args.passes):
        for mode in runs:
            ms, taken = timed_pass(mode, args.steps)
            res[mode].append(round(ms, 4))
            steps_taken[mode].append(taken)
    env = runs['device'][0]
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn, reps):
        torch.cuda.synchronize()
        evs[0].record()
        for _ in range(reps):
            fn()
        evs[1].record()
        torch.cuda.synchronize()
        return evs[0].elapsed_time(evs[1]) * 1000.0 / reps                # us

    env.wait_rs()
    torch.cuda.synchronize()
    action = torch.zeros((n, 2), dtype=env.action_dtype, device=env.device)
    env.eval_begin()                                                      # every scene alive and stuck
    calls = {'k_eval_begin': env.eval_begin, 'k_eval_override': lambda: env.eval_override(action, None, 5, 1), 'k_eval_track': env.eval_track}
    kern = {}
    for name in ('k_eval_begin', 'k_eval_override', 'k_eval_track'):
        fn = calls[name]
        for _ in range(20):
            fn()
        back = timed(fn, args.reps)
        single = sorted(timed(fn, 1) for _ in range(50))
        kern[name] = {'us_back_to_back': round(back, 2), 'us_single_median': round(single[25], 2), 'us_single_min': round(single[0], 2)}
        if name == 'k_eval_begin':
            env.eval_begin()
    es = env.target.element_size()
    kern['k_eval_begin']['bytes_per_scene'] = 5 * es + 16 + 80
    kern['k_eval_override']['bytes_per_scene'] = 8 + 1 + 2 * action.element_size()
    kern['k_eval_track']['bytes_per_scene'] = 160 + 5 * es + 16 + es + 4 + 1 + 8 + 8 + 1
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    spread = {k: round(max(v) - min(v), 4) for k, v in res.items()}
    out = {'scenes': n, 'max_steps_per_pass': args.steps, 'env_steps_taken': steps_taken, 'poll_every': POLL_EVERY, 'ms_per_step': res,
           'ms_per_step_median': med, 'ms_per_step_spread': spread, 'criterion': 'median(device) <= median(torch) + spread(torch)',
           'criterion_met': bool(med['device'] <= med['torch'] + spread['torch']), 'kernels': kern, 'episodes_finished_in_the_last_pass': finished,
           'device': torch.cuda.get_device_name(0), 'arch': env.arch}
    print(json.dumps(out))
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')
    for e, _, _ in runs.values():
        e.close()


if __name__ == '__main__':
    main()
