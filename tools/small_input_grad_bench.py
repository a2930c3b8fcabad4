#!/usr/bin/env python3
"""One training step (forward + H.sum().backward()) with X.requires_grad=True of the un-gated, the time-gated and the node-gated cell at the
two drivers' shapes (epicenter: adj59, F = 20, K = 4; k-step: the N = 50 SBM of fixture G5, F = 20, K = 5; G = 1, B = 64, T = 5 / 20 / 200,
fp32 and fp64): the one-launch small-graph BPTT with its dx variants (ops.small_input_grad_supported) against the composed per-step path
with its autograd replay in the same process (cell._use_small_training = lambda *a: False, the path every tree before the dx variants
takes when X wants a gradient); step time and kernel launches per step.

    python tools/small_input_grad_bench.py [--reps 5] [--iters 20] [--settle-ms 100] [--out profiles/small_input_grad_bench.jsonl]
    python tools/small_input_grad_bench.py --plain [--append]      # the plain training step (X without gradient): run on two commits

What is timed: a host clock around `iters` back-to-back steps (a quarter of that at T = 200) ending in a device synchronise, divided by
the count; `reps` such measurements per path, INTERLEAVED (composed, new, composed, new, ...), each behind untimed steps for --settle-ms
(the clock transient after an idle period). Every sample is written, with median and min .. max per path and ratio = composed median /
new median. Launches: device events of one step under torch.profiler. Acceptance is relative: the new path's median must be below the
composed path's MINIMUM at every configuration (`accepted`). --plain times the step whose X wants no gradient (the entry points that
ran before the dx variants existed), to compare a commit with its parent: `spread` = (max - min) / median of the samples.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from gated_gcrnns_amd import ops
from gated_gcrnns_amd.Utils import graphML

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
SHAPES = {'epicenter_adj59': ('g5_cls_T20K4_none.npz', 4), 'kstep_sbm50': ('g5_reg_multipMlp_none.npz', 5)}
STEPS = (5, 20, 200)
DTYPES = {'f32': torch.float32, 'f64': torch.float64}
CELLS = {'none': (False, None), 'time': (True, None), 'node': (False, 'node')}


def settle(fn, ms):
    t0 = time.perf_counter()
    while ms > 0 and 1e3 * (time.perf_counter() - t0) < ms:
        fn()
        torch.cuda.synchronize()


def step_ms(fn, iters, settle_ms):
    settle(fn, settle_ms)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / iters


def launches(fn):
    from torch.profiler import profile, ProfilerActivity
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def commit():
    try:
        return subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        return None


def summary(v):
    med = statistics.median(v)
    return dict(median_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), spread=round((max(v) - min(v)) / med, 4),
                samples_ms=[round(x, 4) for x in v])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--settle-ms', type=float, default=100.0)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--commit', default=None)
    ap.add_argument('--plain', action='store_true', help='time the training step whose X wants no gradient (no composed comparison)')
    ap.add_argument('--append', action='store_true', help='keep the lines already in --out')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'small_input_grad_bench.jsonl'))
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), 'small_input_grad_bench needs a ROCm device: a CPU timing says nothing about the GPU'
    dev = torch.device('cuda:0')
    rev = args.commit or commit()
    has_new = hasattr(ops, 'small_input_grad_supported')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    lines = []
    if args.append and os.path.exists(args.out):
        lines = [json.loads(ln) for ln in open(args.out) if ln.strip()]
    for sname, (fixture, K) in SHAPES.items():
        S = np.load(os.path.join(GOLDEN, fixture))['S']
        N = S.shape[1]
        for dname, dt in DTYPES.items():
            for cname, (tg, sg) in CELLS.items():
                torch.manual_seed(N + K)
                cell = graphML.GGCRNNCell(1, 20, K, K, torch.tanh, tg, sg, 1, True)
                cell.addGSO(torch.tensor(S))
                cell = cell.to(dev).to(dt)
                for T in STEPS:
                    g = torch.Generator().manual_seed(T)
                    X = torch.randn(args.batch, T, 1, N, generator=g).to(dev, dt).requires_grad_(not args.plain)
                    h0 = torch.zeros(args.batch, 20, N, dtype=dt, device=dev)
                    params = list(cell.parameters())
                    iters = args.iters if T < 200 else max(3, args.iters // 4)

                    def step():
                        for p in params:
                            p.grad = None
                        X.grad = None
                        cell(X, h0).sum().backward()
                        return params + [X]

                    def composed():
                        cell._use_small_training = lambda *a: False
                        try:
                            return step()
                        finally:
                            del cell._use_small_training
                    line = dict(mode='plain' if args.plain else 'dx', shape=sname, N=N, F=20, K=K, G=1, B=args.batch, T=T, dtype=dname,
                                cell=cname, reps=args.reps, iters=iters, settle_ms=args.settle_ms, commit=rev)
                    if args.plain:
                        paths = {'small': step}
                    else:
                        paths = {'composed': composed}
                        if has_new:
                            line['dispatched'] = bool(cell._use_small_training(X, h0))
                            paths['new'] = step
                    times = {k: [] for k in paths}
                    for k, fn in paths.items():
                        for _ in range(3):
                            fn()
                        line[k + '_launches'] = launches(fn)
                    for _ in range(args.reps):                       # interleaved
                        for k, fn in paths.items():
                            times[k].append(step_ms(fn, iters, args.settle_ms))
                    for k, v in times.items():
                        line[k] = summary(v)
                    if 'new' in paths:
                        gn = [p.grad.double().clone() for p in paths['new']() if p.grad is not None]
                        gc = [p.grad.double().clone() for p in paths['composed']() if p.grad is not None]
                        line['max_rel_grad_diff'] = max(float((a - b).abs().max() / (b.abs().max() + 1e-300)) for a, b in zip(gn, gc))
                        line['ratio'] = round(line['composed']['median_ms'] / line['new']['median_ms'], 2)
                        line['accepted'] = bool(line['new']['median_ms'] < line['composed']['min_ms'])
                    lines.append(line)
                    print(json.dumps({k: v for k, v in line.items()}), flush=True)
                    with open(args.out, 'w') as fh:              # rewritten after every row: an interrupted run leaves what it measured
                        for done in lines:
                            fh.write(json.dumps(done) + '\n')
    return lines


if __name__ == '__main__':
    main()
