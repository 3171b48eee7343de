"""HIP-event time of one curriculum tally launch and of one curriculum update (weights + two list fills) at --scenes scenes.

    python tools/curriculum_cost.py --scenes 65536 --reps 200

The tally is timed on the stream of the steps (events around `reps` back-to-back launches on an idle GPU, and around single
launches); the update runs on the handle's pool stream, so its time is taken as the wait of the next step's stream: events around
update + a redraw that must wait for the new lists, minus the same redraw alone.  Last, what the calls cost inside a rollout:
ms per step of `--steps` fused-turnover steps with random actions (a) with the curriculum off, (b) with a tally behind every step,
(c) with an update every 16 steps as well, (d) with a relaxed device refill every 27 steps as well (the step that applies the swap
waits for the incoming set's lists), three passes each, alternating."""
import argparse
import json

import numpy as np
import torch

from hope_amd import ParkingBatch
from hope_amd.scene_gen import mixed_arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenes', type=int, default=65536)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--pool', type=int, default=8192)
    ap.add_argument('--steps', type=int, default=200)
    args = ap.parse_args()
    n = args.scenes
    init = mixed_arrays(2048, levels=('Normal', 'Complex', 'Extrem'), seed=3, max_obst=128)
    env = ParkingBatch(n, 128)
    sl = np.arange(n) % 2048
    env.set_scene_arrays(np.arange(n), init[0][sl], init[1][sl], init[2][sl], init[3][sl], init[4][sl])
    env.set_draw_class(np.arange(3, n, 4), 1)
    env.set_dlp_cases()
    env.generate_pool(args.pool, seed=1)
    env.enable_curriculum()
    env.reset_obs()
    # ~1 % of the scenes finished, as in a rollout
    g = torch.Generator(device='cuda').manual_seed(0)
    env.done.copy_((torch.rand(n, device='cuda', generator=g) < 0.01).to(torch.uint8))
    env.status.copy_(torch.where(env.done.bool(), 3, 1).to(torch.int32))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn, reps):
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1000.0 / reps                  # us

    for _ in range(20):
        env.curriculum_tally()
    tally_stream = timed(env.curriculum_tally, args.reps)
    tally_single = sorted(timed(env.curriculum_tally, 1) for _ in range(50))
    mask = torch.zeros(n, dtype=torch.uint8, device='cuda')               # a redraw of nothing: it only waits for the lists

    def update_and_wait():
        env.curriculum_update()
        env.redraw(mask)

    for _ in range(5):
        update_and_wait()
    wait_only = sorted(timed(lambda: env.redraw(mask), 1) for _ in range(50))
    upd = sorted(timed(update_and_wait, 1) for _ in range(50))
    out = {'scenes': n, 'pool': args.pool, 'n_buckets': env.curriculum_state()['n_buckets'],
           'tally_us_back_to_back': round(tally_stream, 2), 'tally_us_single_median': round(tally_single[25], 2),
           'tally_us_single_min': round(tally_single[0], 2),
           'update_plus_wait_us_median': round(upd[25], 2), 'update_plus_wait_us_min': round(upd[0], 2),
           'empty_redraw_us_median': round(wait_only[25], 2),
           'update_us_median_net': round(upd[25] - wait_only[25], 2)}
    # ---- inside a rollout ----
    env.set_redraw_seed(5)
    acts = [torch.rand((n, 2), device='cuda', generator=g) * 2 - 1 for _ in range(16)]
    batch = [1]

    def rollout(tally, update_every, refill_every):
        for k in range(args.steps):
            if refill_every and k % refill_every == refill_every - 1:
                env.generate_pool(args.pool, seed=1, batch=batch[0], relaxed=True)
                batch[0] += 1
            env.step(acts[k % 16], auto_reset=True, fresh=True, defer_rs=True)
            if tally:
                env.curriculum_tally()
            if update_every and k % update_every == update_every - 1:
                env.curriculum_update()

    modes = {'off': (False, 0, 0), 'tally': (True, 0, 0), 'tally_update16': (True, 16, 0), 'tally_update16_refill27': (True, 16, 27)}
    env.disable_curriculum()
    rollout(False, 0, 0)                                                  # warm-up
    res = {k: [] for k in modes}
    for _ in range(3):
        for name, (tl, ue, rf) in modes.items():
            if tl and not env.curriculum_state()['on']:
                env.enable_curriculum()
            if not tl and env.curriculum_state()['on']:
                env.disable_curriculum()
            res[name].append(round(timed(lambda: rollout(tl, ue, rf), 1) / 1000.0 / args.steps, 4))
    out['rollout_ms_per_step'] = res
    print(json.dumps(out))
    env.close()


if __name__ == '__main__':
    main()
