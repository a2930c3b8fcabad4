#!/usr/bin/env python3
"""Inference forward of the edge-gated and the time+edge-gated cell at the two drivers' shapes (epicenter: adj59, F = 20, K = 4;
k-step: the N = 50 SBM of fixture G5, F = 20, K = 5; G = 1, B = 64, T = 5 / 20 / 200, fp32 and fp64): the one-launch small-graph path
(ops.small_edge_cell_forward) against the composed per-step path in the same process (GCRNN_NO_SMALL_EDGE=1, the path every tree before
this kernel takes), forward time and kernel launches per forward.

    python tools/small_edge_bench.py [--reps 5] [--iters 20] [--settle-ms 100] [--out profiles/small_edge_bench.jsonl]

What is timed: a host clock around `iters` back-to-back forwards ending in a device synchronise, divided by iters; `reps` such
measurements per path, INTERLEAVED (new, composed, new, composed, ...), each behind untimed forwards for --settle-ms (the clock
transient after an idle period). Reported: median and min .. max per path, and ratio = composed median / new median. Launches: device
events of one forward under torch.profiler. On a tree without the kernel only the composed columns are filled (the baseline run).
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


def settle(fn, ms):
    t0 = time.perf_counter()
    while ms > 0 and 1e3 * (time.perf_counter() - t0) < ms:
        fn()
        torch.cuda.synchronize()


def forward_ms(fn, iters, settle_ms):
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


def with_switch(on, fn):
    def run():
        if on:
            os.environ[SWITCH] = '1'
        else:
            os.environ.pop(SWITCH, None)
        try:
            with torch.no_grad():
                return fn()
        finally:
            os.environ.pop(SWITCH, None)
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'small_edge_bench.jsonl'))
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), 'small_edge_bench needs a ROCm device: a CPU timing says nothing about the GPU'
    dev = torch.device('cuda:0')
    rev = args.commit or commit()
    has_new = hasattr(ops, 'small_edge_cell_forward')
    lines = []
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
                    paths = {'composed': with_switch(True, lambda: cell(X, h0))}
                    if has_new:
                        paths['new'] = with_switch(False, lambda: cell(X, h0))
                    line = dict(shape=sname, N=N, F=20, K=K, G=1, B=args.batch, T=T, dtype=dname, cell='time_edge' if tg else 'edge',
                                reps=args.reps, iters=args.iters, settle_ms=args.settle_ms, commit=rev)
                    times = {k: [] for k in paths}
                    for k, fn in paths.items():
                        for _ in range(3):
                            fn()
                        line[k + '_launches'] = launches(fn)
                    for _ in range(args.reps):                       # interleaved
                        for k, fn in paths.items():
                            times[k].append(forward_ms(fn, args.iters, args.settle_ms))
                    for k, v in times.items():
                        line[k] = summary(v)
                    if has_new:
                        line['max_abs_diff'] = float((paths['new']().double() - paths['composed']().double()).abs().max())
                        line['ratio'] = round(line['composed']['median_ms'] / line['new']['median_ms'], 2)
                        line['accepted'] = bool(line['new']['median_ms'] < line['composed']['min_ms'])
                    lines.append(line)
                    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        for line in lines:
            fh.write(json.dumps(line) + '\n')
    return lines


if __name__ == '__main__':
    main()
