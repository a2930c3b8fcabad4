#!/usr/bin/env python3
"""The node gates of the small-graph regime at both drivers' shapes -- epicenter: adj59, K = 4; k-step: SBM N = 80 as
examples/kstep_prediction.py builds it, K = 5; G = 1, F = 20 -- node-gated and time+node-gated, fp32 and fp64, T = 5 / 20 / 200: the cell's
inference forward under no_grad and a full cell training step (zero_grad, forward, L1 on the states, backward, FlatAdam) at B = 64, and the
regression model's (head [1], mlpType='multipMlp') inference at B = 100, with both node gates in one launch forward / one backward (the
default) against GCRNN_NO_SMALL_NODE_GATES=1 (the composed batched pass: node-major pack, four lsigf, tanh, two graph filters, sigmoid,
permute, recorded by autograd) in the same process. The new column runs with GCRNN_SMALL_NODE_GATES=all, so it also times the rows that
GGCRNNCell._small_node_gates_pays leaves to the composed pass.

    python tools/small_node_gates_bench.py [--reps 5] [--iters 20] [--settle-ms 100] [--out profiles/small_node_gates_bench.jsonl] [--append]

Only the public module API and the environment variable are used, so the same file runs on a tree from before the one-launch gates: there
the variable changes nothing, both columns time that tree's only path, and the line carries `has_node_gates_path: false`.

What is timed: a host clock around `iters` back-to-back calls (a quarter of that at T = 200) ending in a device synchronise, divided by the
count; `reps` such measurements per path, INTERLEAVED (off, new, off, new, ...), each behind untimed calls for --settle-ms. Every sample is
written, with median, min .. max and spread = (max - min) / median per path; device events of one call under torch.profiler; and
max_memory_allocated above the allocation before the call. `passes` is the acceptance rule of DESIGN 4.11 / 4.12: new median <= off median
x (1 + off spread)."""
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
from gated_gcrnns_amd.Utils import dataTools, graphML

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
STEPS = (5, 20, 200)
DTYPES = {'f32': torch.float32, 'f64': torch.float64}
GATINGS = {'node': False, 'time+node': True}
SWITCH, EVERY = 'GCRNN_NO_SMALL_NODE_GATES', 'GCRNN_SMALL_NODE_GATES'


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


def switched(fn, off):
    def run():
        if off:
            os.environ[SWITCH] = '1'
        else:
            os.environ.pop(SWITCH, None)
            os.environ[EVERY] = 'all'            # also the rows GGCRNNCell._small_node_gates_pays leaves to the composed pass
        try:
            return fn()
        finally:
            os.environ.pop(SWITCH, None)
            os.environ.pop(EVERY, None)
    return run


def graphs():
    A = np.load(os.path.join(GOLDEN, 'adj59.npy')).reshape(59, 59)
    yield 'epicenter_adj59', A / np.max(np.abs(np.linalg.eigvals(A))), 4
    yield 'kstep_sbm80', dataTools.normalised_gso(dataTools.sbm_adjacency(80, 5, 0.8, 0.2, np.random.default_rng(0))), 5


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--settle-ms', type=float, default=100.0)
    ap.add_argument('--cell-batch', type=int, default=64)
    ap.add_argument('--model-batch', type=int, default=100)
    ap.add_argument('--steps', type=int, nargs='*', default=list(STEPS))
    ap.add_argument('--commit', default=None)
    ap.add_argument('--append', action='store_true', help='keep the lines already in --out')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'small_node_gates_bench.jsonl'))
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), 'small_node_gates_bench needs a ROCm device: a CPU timing says nothing about the GPU'
    dev = torch.device('cuda:0')
    rev = args.commit or commit()
    has_new = hasattr(ops, 'small_node_gates')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    lines = []
    if args.append and os.path.exists(args.out):
        lines = [json.loads(ln) for ln in open(args.out) if ln.strip()]
    F = 20
    for sname, S, K in graphs():
        N = S.shape[-1]
        for dname, dt in DTYPES.items():
            for gname, tg in GATINGS.items():
                torch.manual_seed(N + K)
                cell = graphML.GGCRNNCell(1, F, K, K, torch.tanh, tg, 'node', 1, True)
                cell.addGSO(torch.tensor(np.asarray(S, dtype=np.float64).reshape(1, N, N)))
                cell = cell.to(dev).to(dt)
                copt = optim.make_trainer('ADAM', cell.parameters(), 1e-3, 0.9, 0.999, flat=True)
                torch.manual_seed(N + K)
                model = archit.GatedGCRNNforRegression(1, F, K, K, torch.tanh, torch.nn.ReLU, [1], S, True, time_gating=tg,
                                                       spatial_gating='node', mlpType='multipMlp').to(dev).to(dt)
                for T in args.steps:
                    g = torch.Generator().manual_seed(T)
                    Bc, Bm = args.cell_batch, args.model_batch
                    x = torch.randn(Bm, T, 1, N, generator=g).to(dev, dt)
                    h0 = torch.zeros(Bm, F, N, dtype=dt, device=dev)
                    xc, h0c = x[:Bc].contiguous(), h0[:Bc].contiguous()
                    tgt = torch.randn(Bc, T, F, N, generator=g).to(dev, dt)
                    iters = args.iters if T < 200 else max(3, args.iters // 4)

                    def cell_infer():
                        with torch.no_grad():
                            return cell(xc, h0c)

                    def cell_train():
                        copt.zero_grad()
                        loss = torch.nn.functional.l1_loss(cell(xc, h0c), tgt)
                        loss.backward()
                        copt.step()
                        ops.parameters_changed()
                        return loss

                    def model_infer():
                        with torch.no_grad():
                            return model(x, h0)

                    for mode, fn, B in (('cell_infer', cell_infer, Bc), ('cell_train', cell_train, Bc), ('model_infer', model_infer, Bm)):
                        paths = {'off': switched(fn, True), 'new': switched(fn, False)}
                        line = dict(mode=mode, shape=sname, N=N, F=F, K=K, B=B, T=T, dtype=dname, gating=gname, reps=args.reps, iters=iters,
                                    settle_ms=args.settle_ms, commit=rev, has_node_gates_path=has_new)
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
                        line['passes'] = line['new']['median_ms'] <= line['off']['median_ms'] * (1.0 + line['off']['spread'])
                        lines.append(line)
                        print(json.dumps(line), flush=True)
                        with open(args.out, 'w') as fh:              # rewritten after every row: an interrupted run leaves what it measured
                            for done in lines:
                                fh.write(json.dumps(done) + '\n')
    return lines


if __name__ == '__main__':
    main()
