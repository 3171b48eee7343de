"""What the actor's image token costs on one GPU, in the same run: (a) the torch path, `net.re_embed_img(net.embed_img(img))` eager under
no_grad (MIOpen convolutions; the uint8 -> float32 conversion that precedes it in HopeNet.tokens is part of it), (b)
agent_glue.DeviceImgEncoder (k_imgenc_conv + k_imgenc_head), with the two kernels also timed alone, and (c) agent_glue.DeviceActor end
to end with img_encoder=None against img_encoder='device'.

    python tools/img_encoder_bench.py --out profiles/img_encoder_bench.json

At 8 192 and 65 536 images, each size in a child process of its own under its own time limit (a size that fails ends the run): 5 warm-up
calls of a path, then --reps (default 30) calls, each between two device events; the median, the smallest and the largest are recorded
in microseconds.  `holds` of a row says whether the largest of (b)'s repetitions lies below the smallest of (a)'s.  For the kernels also
their share of the f32 peak (157 TFLOPS, VALU and matrix alike): 2 x 0.82 M multiply-adds per image in the convolutions, 2 x 0.57 M in
the head.  Needs a GPU: there is no fall-back."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32 = 157e12
MAC_CONV = 32 * 32 * 4 * 4 * (27 + 3) + 16 * 16 * 8 * 4 * (36 + 4)
MAC_HEAD = 2048 * 256 + 256 * 128 + 128 * 128


def timed(fn, reps, warmup=5):
    import torch
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


def one_size(n, reps):
    import torch
    from hope_amd import ParkingBatch
    from hope_amd import _lib as L
    from hope_amd import agent_glue as G
    from hope_amd import agents as A
    assert torch.cuda.is_available(), 'needs a HIP device'
    env = ParkingBatch(64, 32)
    dev = env.device
    torch.manual_seed(0)
    ag = A.BatchedPPO(device=dev, use_img=True, state_norm=False)
    net = ag.actor
    g = torch.Generator(device='cpu').manual_seed(n)
    img = torch.randint(0, 256, (n, 3, 64, 64), dtype=torch.uint8, generator=g).to(dev)
    nobs = {'lidar': torch.randn(n, 120, device=dev), 'target': torch.randn(n, 5, device=dev),
            'action_mask': (torch.rand(n, 42, device=dev) < 0.6).float(), 'img': img}
    row = {'images': n, 'device': torch.cuda.get_device_name(0)}

    @torch.no_grad()
    def torch_path():
        return net.re_embed_img(net.embed_img(img.to(torch.float32) * (1.0 / 255.0)))
    row['a_torch'] = timed(torch_path, reps)
    enc = G.DeviceImgEncoder(env, net)
    row['b_device'] = timed(lambda: enc(img), reps)
    token, feat = env.img_encoder_forward(img, features=True)
    args = (C.c_void_p(img.data_ptr()), n, C.c_void_p(token.data_ptr()), C.c_void_p(feat.data_ptr()))
    for stage, name, mac in ((0, 'b_conv_alone', MAC_CONV), (1, 'b_head_alone', MAC_HEAD)):
        row[name] = timed(lambda: L.check(env.lib.hope_debug_imgenc_stage(env.h, stage, *args, env._stream()), 'hope_debug_imgenc_stage'), reps)
        row[name]['fraction_of_f32_peak'] = 2 * mac * n / (row[name]['median_us'] * 1e-6) / PEAK_F32
    row['max_abs_diff_device_vs_torch'] = float((enc(img) - torch_path()).abs().max())
    row['holds'] = row['b_device']['max_us'] < row['a_torch']['min_us']
    row['ratio_of_medians'] = row['a_torch']['median_us'] / row['b_device']['median_us']
    plain, fused = G.DeviceActor(env, net), None
    row['c_actor_torch_encoder'] = timed(lambda: plain(nobs), reps)
    fused = G.DeviceActor(env, net, img_encoder='device')
    row['c_actor_device_encoder'] = timed(lambda: fused(nobs), reps)
    row['max_abs_diff_actor'] = float((fused(nobs) - plain(nobs)).abs().max())
    assert enc.packs == 1 and fused.img_encoder.packs == 1
    env.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='img_encoder_bench.json')
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--sizes', type=int, nargs='+', default=[8192, 65536])
    ap.add_argument('--limit', type=int, default=240, help='seconds a size may take')
    ap.add_argument('--one', type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        print(json.dumps(one_size(args.one, args.reps)))
        return 0
    rows = []
    for n in args.sizes:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--one', str(n), '--reps', str(args.reps)], capture_output=True, text=True,
                               timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(f'{n} images: no result within {args.limit} s; stopping', flush=True)
            return 1
        if r.returncode != 0:
            print(f'{n} images: exit code {r.returncode}; stopping\n{r.stderr[-2000:]}', flush=True)
            return 1
        row = json.loads(r.stdout.strip().splitlines()[-1])
        rows.append(row)
        f = lambda k: f"{row[k]['median_us']:.0f} us [{row[k]['min_us']:.0f}, {row[k]['max_us']:.0f}]"  # noqa: E731
        print(f"{n} images: (a) torch {f('a_torch')}, (b) device {f('b_device')} (conv alone {f('b_conv_alone')}, head alone {f('b_head_alone')}), "
              f"ratio of medians {row['ratio_of_medians']:.1f}, largest (b) below smallest (a): {row['holds']}; (c) actor with the torch encoder "
              f"{f('c_actor_torch_encoder')}, with the device encoder {f('c_actor_device_encoder')}; max |device - torch| token "
              f"{row['max_abs_diff_device_vs_torch']:.2e}, actor {row['max_abs_diff_actor']:.2e}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump({'rows': rows}, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
