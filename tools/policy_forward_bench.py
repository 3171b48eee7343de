"""What the actor's inference forward costs on one GPU on three paths, in the same run: eager `policy_mean` (the torch module, about a
hundred launches), the captured-graph path (`enable_fast_policy(graph=True)`: the same kernels replayed) and agent_glue.DeviceActor (one
fused launch, k_policy_forward).

    python tools/policy_forward_bench.py --out profiles/policy_forward_bench.json

At 8 192 and 65 536 scenes, with T = 3 tokens and with T = 4, where the fourth token is precomputed for all three paths (the image
encoder's convolutions are not part of the comparison): 5 warm-up calls of a path, then --reps (default 30) calls, each between two
device events; the median, the smallest and the largest are recorded in microseconds.  For the device path also its share of the f32
matrix peak (157 TFLOPS): 2 x the multiply-adds of the Linear layers and the attention per scene (1.23 MFLOP at T = 3).  Needs a GPU:
there is no fall-back."""
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
from hope_amd import policy as P  # noqa: E402

PEAK_F32_MATRIX = 157e12


def flop_per_scene(t):
    mac = (120 + 5 + 42) * 128 + 3 * 128 * 128 + t * (128 * 768 + 256 * 128 + 2 * 128 * 128) + 8 * 2 * t * t * 32 + t * 128 * 128 + 128 * 2
    return 2 * mac


class TokenNet(torch.nn.Module):
    """a HopeNet with the image token taken from the observation ('img_token') instead of the encoder"""

    def __init__(self, net):
        super().__init__()
        self.inner = net

    def forward(self, x):
        n = self.inner
        f = [n.embed_lidar(x['lidar']), n.embed_tgt(x['target']), n.embed_am(x['action_mask'])]
        if 'img_token' in x:
            f.append(x['img_token'])
        out = n.net(torch.stack(f, dim=1))
        return torch.tanh(out) if n.tanh_out else out


def timed(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return {'median_us': statistics.median(us), 'min_us': min(us), 'max_us': max(us), 'reps': reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='policy_forward_bench.json')
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--sizes', type=int, nargs='+', default=[8192, 65536])
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a HIP device'
    res = {'device': torch.cuda.get_device_name(0), 'rows': []}
    for t in (3, 4):
        env = ParkingBatch(64, 32)
        dev = env.device
        torch.manual_seed(0)
        ag = A.BatchedPPO(device=dev, use_img=t == 4, state_norm=False)
        net = ag.actor
        ag.actor = TokenNet(net)
        dact = G.DeviceActor(env, net)
        for n in args.sizes:
            nobs = {'lidar': torch.randn(n, 120, device=dev), 'target': torch.randn(n, 5, device=dev),
                    'action_mask': (torch.rand(n, 42, device=dev) < 0.6).float()}
            if t == 4:
                nobs['img_token'] = torch.randn(n, 128, device=dev)
            row = {'scenes': n, 'tokens': t}
            ag.disable_fast_policy()
            row['eager'] = timed(lambda: ag.policy_mean(nobs), args.reps)
            ag.enable_fast_policy(graph=True)
            row['graph'] = timed(lambda: ag.policy_mean(nobs), args.reps)
            ag.disable_fast_policy()
            row['device'] = timed(lambda: dact(nobs), args.reps)
            row['device_kernel_only'] = timed(lambda: env.policy_forward(nobs['lidar'], nobs['target'], nobs['action_mask'], nobs.get('img_token')), args.reps)
            row['max_abs_diff_device_vs_eager'] = float((dact(nobs) - ag.policy_mean(nobs)).abs().max())
            fl = flop_per_scene(t) * n
            row['device_fraction_of_f32_matrix_peak'] = fl / (row['device_kernel_only']['median_us'] * 1e-6) / PEAK_F32_MATRIX
            res['rows'].append(row)
            print(f"T={t} scenes={n}: eager {row['eager']['median_us']:.0f} us [{row['eager']['min_us']:.0f}, {row['eager']['max_us']:.0f}], "
                  f"graph {row['graph']['median_us']:.0f} us [{row['graph']['min_us']:.0f}, {row['graph']['max_us']:.0f}], "
                  f"device {row['device']['median_us']:.0f} us [{row['device']['min_us']:.0f}, {row['device']['max_us']:.0f}] "
                  f"(kernel alone {row['device_kernel_only']['median_us']:.0f} us, {100 * row['device_fraction_of_f32_matrix_peak']:.1f} % of the f32 matrix peak), "
                  f"max |device - eager| {row['max_abs_diff_device_vs_eager']:.2e}", flush=True)
        assert dact.packs == 1
        env.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
