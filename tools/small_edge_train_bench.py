#!/usr/bin/env python3
"""One training step (forward + H.sum().backward()) of the edge-gated and the time+edge-gated cell at the two drivers' shapes (epicenter:
adj59, F = 20, K = 4; k-step: the N = 50 SBM of fixture G5, F = 20, K = 5; G = 1, B = 64, T = 5 / 20 / 200, fp32 and fp64): the small-graph
training path (ops.small_edge_cell_train: two launches forward, two backward) against the composed per-step path with its autograd replay
in the same process (GCRNN_NO_SMALL_EDGE=1, the path every tree before these kernels takes); step time and kernel launches per step.

    python tools/small_edge_train_bench.py [--reps 5] [--iters 20] [--settle-ms 100] [--out profiles/small_edge_train_bench.jsonl]
    python tools/small_edge_train_bench.py --x-grad [...] [--out profiles/small_edge_input_grad_bench.jsonl]

--x-grad: the step's X requires a gradient (a stacked cell, an encoder in front, saliency). New path: GCRNN_SMALL_EDGE_DX=1 (the BPTT
kernels' dx variant, ops.small_edge_input_grad_supported); composed path: the variable unset, which is what the module does by default
and what every tree before the dx variant does. X.grad is part of the compared gradients.

What is timed: a host clock around `iters` back-to-back steps ending in a device synchronise, divided by iters; `reps` such
measurements per path, INTERLEAVED (composed, new, composed, new, ...), each behind untimed steps for --settle-ms (the clock
transient after an idle period). Reported: median and min .. max per path, and ratio = composed median / new median. Launches: device
events of one step under torch.profiler. On a tree without the kernels only the composed columns are filled (the baseline run).
Acceptance is relative: the new path's median must be below the composed path's MINIMUM at every shape (`accepted`).
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
SWITCH = 'GCRNN_NO_SMALL_EDGE'
DX_SWITCH = 'GCRNN_SMALL_EDGE_DX'


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


def with_switch(on, fn, name=SWITCH):
    def run():
        if on:
            os.environ[name] = '1'
        else:
            os.environ.pop(name, None)
        try:
            return fn()
        finally:
            os.environ.pop(name, None)
    return run


def commit():
    try:
        return subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        return None


def summary(v):
    return dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--settle-ms', type=float, default=100.0)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--commit', default=None)
    ap.add_argument('--x-grad', action='store_true', help='X requires a gradient; new path = GCRNN_SMALL_EDGE_DX=1, composed = unset')
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    if args.out is None:
        args.out = os.path.join(ROOT, 'profiles', 'small_edge_input_grad_bench.jsonl' if args.x_grad else 'small_edge_train_bench.jsonl')
    assert torch.cuda.is_available(), 'small_edge_train_bench needs a ROCm device: a CPU timing says nothing about the GPU'
    dev = torch.device('cuda:0')
    rev = args.commit or commit()
    has_new = hasattr(ops, 'small_edge_input_grad_supported' if args.x_grad else 'small_edge_cell_train')
    lines = []
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for sname, (fixture, K) in SHAPES.items():
        S = np.load(os.path.join(GOLDEN, fixture))['S']
        N = S.shape[1]
        for dname, dt in DTYPES.items():
            for tg in (False, True):
                torch.manual_seed(N + K)
                cell = graphML.GGCRNNCell(1, 20, K, K, torch.tanh, tg, 'edge', 1, True)
                cell.addGSO(torch.tensor(S))
                cell = cell.to(dev).to(dt)
                for T in STEPS:
                    g = torch.Generator().manual_seed(T)
                    X = torch.randn(args.batch, T, 1, N, generator=g).to(dev, dt)
                    h0 = torch.zeros(args.batch, 20, N, dtype=dt, device=dev)
                    params = list(cell.parameters())
                    if args.x_grad:
                        params.append(X.requires_grad_())

                    def step():
                        for p in params:
                            p.grad = None
                        cell(X, h0).sum().backward()
                        return params
                    if args.x_grad:
                        os.environ.pop(SWITCH, None)
                        paths = {'composed': with_switch(False, step, DX_SWITCH)}
                        if has_new:
                            paths['new'] = with_switch(True, step, DX_SWITCH)
                    else:
                        paths = {'composed': with_switch(True, step)}
                        if has_new:
                            paths['new'] = with_switch(False, step)
                    line = dict(shape=sname, N=N, F=20, K=K, G=1, B=args.batch, T=T, dtype=dname, cell='time_edge' if tg else 'edge',
                                reps=args.reps, iters=args.iters, settle_ms=args.settle_ms, commit=rev, **({'x_grad': True} if args.x_grad else {}))
                    times = {k: [] for k in paths}
                    for k, fn in paths.items():
                        for _ in range(3):
                            fn()
                        line[k + '_launches'] = launches(fn)
                    for _ in range(args.reps):                       # interleaved
                        for k, fn in paths.items():
                            times[k].append(step_ms(fn, args.iters, args.settle_ms))
                    for k, v in times.items():
                        line[k] = summary(v)
                    if has_new:
                        gn = [p.grad.double().clone() for p in paths['new']() if p.grad is not None]
                        gc = [p.grad.double().clone() for p in paths['composed']() if p.grad is not None]
                        line['max_rel_grad_diff'] = max(float((a - b).abs().max() / (b.abs().max() + 1e-300)) for a, b in zip(gn, gc))
                        line['ratio'] = round(line['composed']['median_ms'] / line['new']['median_ms'], 2)
                        line['accepted'] = bool(line['new']['median_ms'] < line['composed']['min_ms'])
                    lines.append(line)
                    print(json.dumps(line), flush=True)
                    with open(args.out, 'w') as fh:              # rewritten after every row: an interrupted run leaves what it measured
                        for done in lines:
                            fh.write(json.dumps(done) + '\n')
    return lines


if __name__ == '__main__':
    main()
