"""Event-times hope_env_map_level on the bench's scene mix (Normal / Complex / Extrem / dlp round-robin, 2 048 unique scenes tiled)
and times the route the library had before -- download_scenes + Python get_map_level -- on a sample; prints one JSON line.
    python tools/map_level_timing.py [--scenes 65536] [--sample 64]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hope_amd import ParkingBatch, map_level as M                                # noqa: E402
from hope_amd.scene_gen import mixed_arrays                                     # noqa: E402

LEVELS = ('Normal', 'Complex', 'Extrem', 'dlp')


def event_ms(fn, reps=20):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenes', type=int, default=65536)
    ap.add_argument('--unique', type=int, default=2048)
    ap.add_argument('--sample', type=int, default=64, help='scenes per class for the Python timing')
    args = ap.parse_args()
    n, u = args.scenes, min(args.scenes, args.unique)
    arr = mixed_arrays(u, levels=LEVELS, seed=0, max_obst=128)
    sl = np.arange(n) % u
    env = ParkingBatch(n, 128)
    env.set_scene_arrays(np.arange(n), *[a[sl] for a in arr[:5]])
    out = torch.zeros(n, dtype=torch.uint8, device='cuda')
    det = torch.zeros((n, 8), dtype=torch.int32, device='cuda')
    res = {'scenes': n, 'total_ms': event_ms(lambda: env.map_levels(out=out)), 'total_detail_ms': event_ms(lambda: env.map_levels(out=out, detail=det))}
    res['us_per_scene'] = res['total_ms'] * 1e3 / n
    cls = torch.arange(n, device='cuda') % u % 4
    for k, name in enumerate(LEVELS):
        mask = (cls == k).to(torch.uint8)
        res[f'{name}_ms'] = event_ms(lambda: env.map_levels(active=mask, out=out))
        ids = np.nonzero(mask.cpu().numpy())[0][:args.sample]
        t0 = time.perf_counter()
        start, dest, _, verts, nob = env.download_scenes(ids)
        for j in range(len(ids)):
            M.get_map_level(start[j], dest[j], [verts[j, o] for o in range(int(nob[j]))])
        res[f'{name}_python_us_per_scene'] = (time.perf_counter() - t0) * 1e6 / len(ids)
        res[f'{name}_mean_obstacles'] = float(nob.mean())
    res['python_us_per_scene'] = float(np.mean([res[f'{name}_python_us_per_scene'] for name in LEVELS]))
    res['ratio'] = res['python_us_per_scene'] / res['us_per_scene']
    t0 = time.perf_counter()
    start, dest, _, verts, nob = env.download_scenes(np.arange(min(n, 4096)))
    t1 = time.perf_counter()
    M.get_map_levels_host(start, dest, verts, nob)
    res['host_core_us_per_scene'] = (time.perf_counter() - t1) * 1e6 / len(nob)
    res['download_us_per_scene'] = (t1 - t0) * 1e6 / len(nob)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
