#!/usr/bin/env python3
"""What does a pool refill cost, drawn on the device (k_scenegen, hope_env_generate_pool) against drawn on the host?
Prints, for a pool of --pool lots at max_obst 128:
  * the device generator: time per refill (host clock from the call to the completed swap, the handle otherwise idle) and the
    kernel alone (device events around hope_scenegen_generate_device, one launch per level), lots/s;
  * the host twin (hope_scenegen_generate_det) and the glibc generator (hope_scenegen_generate) on 1 and 2 threads;
  * ms per step of a --scenes batch (bench.py's configuration: mixed levels, HOPE_AUTO_REDRAW, deferred search) over windows of
    --window steps with (a) no refresh, (b) PoolRefresher driven as bench.py drives it, (c) DevicePoolRefresher at the same
    period; the three alternate --rounds times; per-step device times (events) give the median / p99 / worst step of a window.
    python tools/scenegen_cost.py > profiles/scenegen_cost.txt"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEVELS = ('Normal', 'Complex', 'Extrem')


def host_rate(fn, n_pool, mo, threads, reps=5):
    best = 1e9
    for r in range(reps):
        t0 = time.perf_counter()
        for j, lv in enumerate(LEVELS):
            fn(lv, n_pool // 3, seed=100 + j, max_obst=mo, first_index=r * n_pool, threads=threads)
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenes', type=int, default=65536)
    ap.add_argument('--pool', type=int, default=8192)
    ap.add_argument('--window', type=int, default=540)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--threads', type=int, default=2)
    a = ap.parse_args()
    import torch
    from hope_amd import ParkingBatch
    from hope_amd.scene_gen import (DevicePoolRefresher, PoolRefresher, generate_arrays, generate_arrays_det, generate_arrays_device,
                                    mixed_arrays)
    assert torch.cuda.is_available(), 'needs a HIP device'
    N, P, mo = a.scenes, a.pool // 3 * 3, 128
    out = {'scenes': N, 'pool': P, 'max_obst': mo}

    # ---- host generators ------------------------------------------------------------------------------------------
    generate_arrays('Normal', 512, max_obst=mo); generate_arrays_det('Normal', 512, max_obst=mo)
    for name, fn in (('glibc', generate_arrays), ('twin', generate_arrays_det)):
        for th in (1, 2):
            s = host_rate(fn, P, mo, th)
            out[f'host_{name}_{th}thr_ms'] = round(s * 1e3, 3)
            out[f'host_{name}_{th}thr_lots_per_s'] = round(P / s)

    # ---- the kernel alone -----------------------------------------------------------------------------------------
    bufs = {lv: generate_arrays_device(lv, P // 3, seed=1, max_obst=mo) for lv in LEVELS}       # warm-up: code object, buffers
    torch.cuda.synchronize()
    ks = []
    for r in range(10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for j, lv in enumerate(LEVELS):
            generate_arrays_device(lv, P // 3, seed=100 + j, max_obst=mo, first_index=r * P, out=bufs[lv])
        e1.record()
        torch.cuda.synchronize()
        ks.append(e0.elapsed_time(e1))
    out['device_kernels_ms_median'] = round(float(np.median(ks)), 4)
    out['device_kernels_ms_min_max'] = [round(min(ks), 4), round(max(ks), 4)]
    out['device_kernels_lots_per_s'] = round(P / (np.median(ks) * 1e-3))
    del bufs

    # ---- three batches as bench.py sets its own up, one per refresh mode (a handle with a host refresher always has a staging
    # fill in flight, which hope_env_generate_pool refuses, so the modes do not share a handle) ----------------------------
    levels = LEVELS + ('dlp',)
    U = 2048
    start, dest, bbox, verts, nob, nvert = mixed_arrays(U, levels=levels, seed=42, max_obst=mo)
    parts = [generate_arrays(lv, P // 3, seed=17 + j, max_obst=mo) for j, lv in enumerate(LEVELS)]
    first_pool = tuple(np.concatenate([p_[j] for p_ in parts]) for j in range(6))
    g = torch.Generator(device='cuda').manual_seed(1)
    acts = [torch.rand((N, 2), device='cuda', generator=g) * 2 - 1 for _ in range(64)]

    def make_env():
        env = ParkingBatch(N, mo, obs_dtype=torch.float32, action_dtype=torch.float32)
        for s0 in range(0, N, 8192):
            ids = np.arange(s0, min(N, s0 + 8192))
            sl = ids % U
            env.set_scene_arrays(ids, start[sl], dest[sl], bbox[sl], verts[sl], nob[sl])
        env.set_draw_class(np.nonzero(np.arange(N) % U % 4 == 3)[0], 1)
        env.set_pool(first_pool)
        env.set_dlp_cases()
        env.set_redraw_seed(7)
        env.reset_obs()
        for i in range(300):                                 # pre-roll: a steady age mix
            env.step(acts[i % len(acts)], auto_reset=True, fresh=True, defer_rs=True)
        torch.cuda.synchronize()
        return env
    envs = {mode: make_env() for mode in ('none', 'host', 'device')}

    # ---- one refill on an otherwise idle handle: call -> swap complete ----------------------------------------------
    env = envs['device']
    env.generate_pool(P, LEVELS, seed=3, batch=0)
    env.pool_generation(); torch.cuda.synchronize()
    rf = []
    for r in range(10):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        env.generate_pool(P, LEVELS, seed=3, batch=1 + r, relaxed=True)
        t1 = time.perf_counter()
        env.pool_generation()                                # applies the relaxed swap: waits for the generator's event
        t2 = time.perf_counter()
        rf.append(((t1 - t0) * 1e3, (t2 - t0) * 1e3))
    out['device_refill_call_ms_median'] = round(float(np.median([x[0] for x in rf])), 4)
    out['device_refill_complete_ms_median'] = round(float(np.median([x[1] for x in rf])), 4)
    out['device_refill_lots_per_s'] = round(P / (np.median([x[1] for x in rf]) * 1e-3))

    # ---- step time with and without refresh --------------------------------------------------------------------------
    every = max(8, int(P / (0.0045 * N)))
    out['refresh_every_steps'] = every
    host_ref = PoolRefresher(envs['host'], P, levels=LEVELS, seed=11, relaxed=False, threads=a.threads)
    dev_ref = DevicePoolRefresher(envs['device'], P, levels=LEVELS, seed=11, relaxed=False)
    clock = {'none': 0, 'host': 0, 'device': 0}

    def window(mode):
        env = envs[mode]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.window + 1)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record()
        for i in range(a.window):
            env.step(acts[clock[mode] % len(acts)], auto_reset=True, fresh=True, defer_rs=True)
            ph = clock[mode] % every
            if mode == 'host':                               # bench.py's schedule: commit at the period's end, fill as soon as the staging is free
                if ph == 0 and host_ref.thread is not None:
                    host_ref.poll(wait=True)
                if host_ref.thread is None:
                    host_ref.start_fill(block=ph >= every // 2)
            elif mode == 'device' and ph == 0:
                dev_ref.poll()
            clock[mode] += 1
            ev[i + 1].record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3 / a.window
        per = np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(a.window)])
        return {'ms_per_step': round(wall, 4), 'median': round(float(np.median(per)), 4), 'p99': round(float(np.percentile(per, 99)), 4),
                'max': round(float(per.max()), 4)}
    for mode in envs:                                        # warm every path once
        window(mode)
    res = {mode: [] for mode in envs}
    for r in range(a.rounds):
        for mode in envs:
            res[mode].append(window(mode))
    out['windows'] = res
    out['host_refresher_commits'] = host_ref.commits
    out['device_refresher_commits'] = dev_ref.commits
    out['pool_overflow'] = [e.pool_overflow() for e in envs.values()]
    host_ref.close()
    for e in envs.values():
        e.close()
    for k, v in out.items():
        print(k, json.dumps(v))


if __name__ == '__main__':
    main()
