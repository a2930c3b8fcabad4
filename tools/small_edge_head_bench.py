#!/usr/bin/env python3
"""The edge-gated models of both drivers on small graphs -- GatedGCRNNforClassification (adj59, F = 20, K = 4, head [11]) and
GatedGCRNNforRegression (SBM N = 50 as examples/kstep_prediction.py builds it, F = 20, K = 5, head [1], mlpType='multipMlp'; N = 50 is
the driver's graph size at which the fp64 edge-gated BPTT image still fits in LDS), edge and time+edge gating, fp32 and fp64,
B = 100, T = 5 / 20 / 200: the inference forward under no_grad and a full training step (zero_grad, forward, loss, backward, FlatAdam),
with the head inside the edge-gated recurrence launches (GCRNN_SMALL_EDGE_HEAD=all: every supported row) against the two-module path
(the variable unset) in the same process.

    python tools/small_edge_head_bench.py [--reps 5] [--iters 20] [--settle-ms 100] [--out profiles/small_edge_head_bench.jsonl] [--append]

Only the public module API and the environment variable are used, so the same file runs on a tree from before the heads: there the
variable changes nothing, both columns time that tree's only path, and the line carries `has_head_path: false`. That is how the parent's own
figures are taken on the same machine.

What is timed: a host clock around `iters` back-to-back calls (a quarter of that at T = 200) ending in a device synchronise, divided by the
count; `reps` such measurements per path, INTERLEAVED (off, new, off, new, ...), each behind untimed calls for --settle-ms. Every sample is
written, with median, min .. max and spread = (max - min) / median per path; device events of one call under torch.profiler; and
max_memory_allocated above the allocation before the call."""
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

from gated_gcrnns_amd import ops, optim
from gated_gcrnns_amd.Modules import architectures as archit
from gated_gcrnns_amd.Utils import dataTools, miscTools

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
STEPS = (5, 20, 200)
DTYPES = {'f32': torch.float32, 'f64': torch.float64}
GATINGS = {'edge': False, 'time+edge': True}
SWITCH = 'GCRNN_SMALL_EDGE_HEAD'


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


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def commit():
    try:
        return subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        return None


def summary(v):
    med = statistics.median(v)
    return dict(median_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), spread=round((max(v) - min(v)) / med, 4),
                samples_ms=[round(x, 4) for x in v])


def switched(fn, on):
    def run():
        if on:
            os.environ[SWITCH] = 'all'                       # every supported row, also those GGCRNNCell._small_edge_head_pays takes off =1
        else:
            os.environ.pop(SWITCH, None)
        try:
            return fn()
        finally:
            os.environ.pop(SWITCH, None)
    return run


def models():
    """(model kind, N, F, K, width of the head, GSO) of the two drivers."""
    A = np.load(os.path.join(GOLDEN, 'adj59.npy')).reshape(59, 59)
    yield 'classification', 59, 20, 4, 11, A / np.max(np.abs(np.linalg.eigvals(A)))
    S = dataTools.normalised_gso(dataTools.sbm_adjacency(50, 5, 0.8, 0.2, np.random.default_rng(0)))     # examples/kstep_prediction.py:71-72
    yield 'regression', 50, 20, 5, 1, S


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--settle-ms', type=float, default=100.0)
    ap.add_argument('--batch', type=int, default=100)
    ap.add_argument('--steps', type=int, nargs='*', default=list(STEPS))
    ap.add_argument('--dtypes', nargs='*', default=list(DTYPES), choices=list(DTYPES))
    ap.add_argument('--models', nargs='*', default=['classification', 'regression'])
    ap.add_argument('--gatings', nargs='*', default=list(GATINGS), choices=list(GATINGS))
    ap.add_argument('--modes', nargs='*', default=['infer', 'train'], choices=['infer', 'train'])
    ap.add_argument('--commit', default=None)
    ap.add_argument('--append', action='store_true', help='keep the lines already in --out')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'small_edge_head_bench.jsonl'))
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), 'small_edge_head_bench needs a ROCm device: a CPU timing says nothing about the GPU'
    dev = torch.device('cuda:0')
    rev = args.commit or commit()
    has_new = hasattr(ops, 'small_edge_cell_classify')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    lines = []
    if args.append and os.path.exists(args.out):
        lines = [json.loads(ln) for ln in open(args.out) if ln.strip()]
    for kind, N, F, K, W, S in models():
        if kind not in args.models:
            continue
        for dname in args.dtypes:
            dt = DTYPES[dname]
            for gname in args.gatings:
                tg = GATINGS[gname]
                torch.manual_seed(N + K)
                if kind == 'classification':
                    m = archit.GatedGCRNNforClassification(1, F, K, K, torch.tanh, torch.nn.ReLU, [W], S, True, time_gating=tg, spatial_gating='edge')
                else:
                    m = archit.GatedGCRNNforRegression(1, F, K, K, torch.tanh, torch.nn.ReLU, [W], S, True, time_gating=tg, spatial_gating='edge',
                                                       mlpType='multipMlp')
                m = m.to(dev).to(dt)
                opt = optim.make_trainer('ADAM', m.parameters(), 1e-3, 0.9, 0.999, flat=True)
                for T in args.steps:
                    g = torch.Generator().manual_seed(T)
                    x = torch.randn(args.batch, T, 1, N, generator=g).to(dev, dt)
                    h0 = torch.zeros(args.batch, F, N, dtype=dt, device=dev)
                    if kind == 'classification':
                        y = torch.randint(0, W, (args.batch,), generator=g).to(dev)
                    else:
                        y = torch.randn(args.batch, T, 1, N, generator=g).to(dev, dt)
                    iters = args.iters if T < 200 else max(3, args.iters // 4)

                    def infer():
                        with torch.no_grad():
                            return m(x, h0)

                    def train():
                        opt.zero_grad()
                        out = m(x, h0)
                        loss = ops.cross_entropy(out, y) if kind == 'classification' else miscTools.batchTimeL1Loss(out, y)
                        loss.backward()
                        opt.step()
                        ops.parameters_changed()
                        return loss

                    for mode, fn in (('infer', infer), ('train', train)):
                        if mode not in args.modes:
                            continue
                        paths = {'off': switched(fn, False), 'new': switched(fn, True)}
                        line = dict(model=kind, mode=mode, N=N, F=F, K=K, head=W, B=args.batch, T=T, dtype=dname, gating=gname, reps=args.reps,
                                    iters=iters, settle_ms=args.settle_ms, commit=rev, has_head_path=has_new)
                        times = {k: [] for k in paths}
                        for k, run in paths.items():
                            for _ in range(3):
                                run()
                            line[k + '_launches'] = launches(run)
                            line[k + '_peak_bytes'] = peak_bytes(run)
                        for _ in range(args.reps):                       # interleaved
                            for k, run in paths.items():
                                times[k].append(step_ms(run, iters, args.settle_ms))
                        for k, v in times.items():
                            line[k] = summary(v)
                        line['ratio'] = round(line['off']['median_ms'] / line['new']['median_ms'], 3)
                        lines.append(line)
                        print(json.dumps(line), flush=True)
                        with open(args.out, 'w') as fh:              # rewritten after every row: an interrupted run leaves what it measured
                            for done in lines:
                                fh.write(json.dumps(done) + '\n')
    return lines


if __name__ == '__main__':
    main()
