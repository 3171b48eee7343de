"""What the optimiser block of an update costs on one GPU, torch's own path against agent_glue.DeviceAdam / DevicePolyak, in the same run:

  sac_block        critic_opt1.step(), critic_opt2.step(), actor_opt.step(), alpha_opt.step() (ONE float64 scalar) and the two
                   _soft_updates of BatchedSAC.update, as the agent constructs them -- without the image token, then with it;
  ppo_pair         actor_opt.step(), critic_opt.step() of one BatchedPPO minibatch;
  ppo_soft_update  its one _soft_update per epoch.

    python tools/optim_step_bench.py --out profiles/optim_step_bench.json

The baseline is `torch.optim.Adam.step()` and `agents._soft_update` on the same tensors with the same gradients, eager and -- where the
capture succeeds -- as one captured graph of the same kernels (a capture bakes the step count in: it measures the launches, it is not
a way to train).  The device path is step_optimizers / DevicePolyak over copies of the same nets.  Every path is warmed up; then --reps
(default 10) repetitions, in each of which every path is timed in turn (alternating, so that a drift of the machine touches all of
them) over a window of several back-to-back calls between two device events; the smallest, the median and the largest per-call time
of the repetitions are recorded in microseconds.  The launch counts of one call of either path are what torch.profiler counts on the
device.  Needs a GPU: there is no fall-back."""
import argparse
import copy
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
    """fn's kernels as one captured graph -> replay, or None and why not"""
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        return g.replay, None
    except Exception as e:  # noqa: BLE001 -- whatever the capture refuses is the finding
        torch.cuda.synchronize()
        return None, f'{type(e).__name__}: {str(e).splitlines()[0][:200]}'


def launches(fn):
    """(kernels, copies and memsets) one call of fn puts on the device, as torch.profiler counts them -- or None and why not"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        other = [e for e in dev if 'memcpy' in e.name.lower() or 'memset' in e.name.lower()]
        return {'kernels': len(dev) - len(other), 'copies_and_memsets': len(other)}
    except Exception as e:  # noqa: BLE001
        return {'error': f'{type(e).__name__}: {str(e).splitlines()[0][:200]}'}


def fill_grads(params, seed):
    g = torch.Generator(device='cpu').manual_seed(seed)
    for p in params:
        p.grad = (torch.randn(p.shape, generator=g, dtype=p.dtype) * 1e-2).to(p.device)


def sac_paths(env, use_img):
    torch.manual_seed(0)
    base = A.BatchedSAC(device=env.device, use_img=use_img, state_norm=False)
    dev = copy.deepcopy(base)
    for ag in (base, dev):                            # (deepcopy keeps the optimisers bound to the copies' own parameters)
        ps = [p for o in (ag.critic_opt1, ag.critic_opt2, ag.actor_opt, ag.alpha_opt) for g in o.param_groups for p in g['params']]
        fill_grads(ps, 1)
    G.make_optimizers('device', env, dev)

    def eager():
        base.critic_opt1.step()
        base.critic_opt2.step()
        base.actor_opt.step()
        base.alpha_opt.step()
        A._soft_update(base.critic_target1, base.critic1, base.tau)
        A._soft_update(base.critic_target2, base.critic2, base.tau)

    def device():
        G.step_optimizers(dev.critic_opt1, dev.critic_opt2)
        dev.actor_opt.step()
        dev.alpha_opt.step()
        dev._soft_updates()
    tensors = sum(len(list(n.parameters())) for n in (base.critic1, base.critic2, base.actor)) + 2
    elements = sum(p.numel() for n in (base.critic1, base.critic2, base.actor) for p in n.parameters()) + 3
    return eager, device, (base, dev), {'tensors_stepped': tensors, 'elements_stepped': elements}


def ppo_paths(env):
    torch.manual_seed(0)
    base = A.BatchedPPO(device=env.device, use_img=False, state_norm=False)
    dev = copy.deepcopy(base)
    for ag in (base, dev):
        fill_grads([p for o in (ag.actor_opt, ag.critic_opt) for g in o.param_groups for p in g['params']], 1)
    G.make_optimizers('device', env, dev)
    pair = (lambda: (base.actor_opt.step(), base.critic_opt.step()), lambda: G.step_optimizers(dev.actor_opt, dev.critic_opt))
    soft = (lambda: A._soft_update(base.critic_target, base.critic, base.tau), lambda: dev.soft_update([(dev.critic_target, dev.critic)], dev.tau))
    n = {'tensors_stepped': len(base.trainable()), 'elements_stepped': sum(p.numel() for p in base.trainable())}
    return pair, soft, (base, dev), n


def max_diff(base, dev, names):
    return max(float((p.detach().double() - q.detach().double()).abs().max()) for k in names for p, q in zip(getattr(base, k).parameters(), getattr(dev, k).parameters()))


def show(row):
    parts = [f"{k} {v['median_us']:.0f} us [{v['min_us']:.0f}, {v['max_us']:.0f}]" for k, v in row.items() if isinstance(v, dict) and 'median_us' in v]
    print(f"{row['what']}: " + ', '.join(parts) + f"; launches eager {row['launches_eager']}, device {row['launches_device']}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='optim_step_bench.json')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--no-graph', action='store_true', help='skip the captured-graph baseline')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a HIP device'
    res = {'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'rows': []}
    env = ParkingBatch(64, 32)

    def measure(what, eager, device, extra):
        row = dict({'what': what}, **extra)
        paths = {'eager': eager, 'device': device}
        if not args.no_graph:
            replay, why = captured(eager)
            if replay is not None:
                paths['graph'] = replay
            else:
                row['graph_not_captured'] = why
        row.update(compare(paths, args.reps, args.calls))
        row['launches_eager'], row['launches_device'] = launches(eager), launches(device)
        res['rows'].append(row)
        show(row)
        return row

    for use_img in (False, True):
        eager, device, (base, dev), n = sac_paths(env, use_img)
        row = measure('sac_block' + ('_img' if use_img else ''), eager, device, n)
        # both sides have taken the same number of steps only up to the warm-ups' difference: the distance is reported, not asserted
        row['max_abs_param_diff_device_vs_eager'] = max_diff(base, dev, ('critic1', 'actor', 'critic_target1'))
    pair, soft, (base, dev), n = ppo_paths(env)
    measure('ppo_pair', pair[0], pair[1], n)
    measure('ppo_soft_update', soft[0], soft[1], {'tensors_stepped': len(list(base.critic.parameters())), 'elements_stepped': sum(p.numel() for p in base.critic.parameters())})
    env.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
