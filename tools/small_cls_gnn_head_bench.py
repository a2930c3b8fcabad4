#!/usr/bin/env python3
"""The classification model with a one-layer Selection-GNN head (GatedGCRNNforClassification, dimNodeSignals = [20, 1],
nFilterTaps = [4], ReLU, NoPool, dimLayersMLP = [11]: the epicenter driver's GCRNNGNN) at the driver's shape -- adj59, F = 20,
K = K_o = 4, C = 11, B = 100, T = 5 / 20 / 200, fp32 and fp64, un-gated, time-gated and node-gated: the inference forward under no_grad and
a full training step (zero_grad, forward, cross-entropy, backward, FlatAdam), with the head inside the small-graph launches (the new
path, GCRNN_SMALL_CLS_GNN_HEAD=all) against GCRNN_NO_SMALL_CLS_GNN_HEAD=1 (the cell's launches, `select`, then SelectionGNN as a separate
module) in the same process.

    python tools/small_cls_gnn_head_bench.py [--reps 5] [--iters 20] [--settle-ms 100] [--out profiles/small_cls_gnn_head_bench.jsonl] [--append]

Only the public module API and the environment variables are used, so the same file runs on a tree from before the in-launch head: there
the variables change nothing, both columns time that tree's only path, and the line carries `has_head_path: false`.

What is timed: as tools/small_gnn_head_bench.py (its helpers and those of tools/small_cls_bench.py are used) -- a host clock around `iters`
back-to-back calls ending in a device synchronise, `reps` such measurements per path, INTERLEAVED (off, new, off, new, ...), each behind
untimed calls for --settle-ms. Every sample is written, with median, min .. max and spread = (max - min) / median per path; the device
events of one call under torch.profiler (their count and summed device time); and max_memory_allocated above the allocation before the
call. `passes`: the acceptance rule of DESIGN 4.14, new median <= off median x (1 + off spread), which
GGCRNNCell._small_cls_gnn_head_pays follows."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import torch

import small_cls_bench as scb
from small_gnn_head_bench import device_events
from gated_gcrnns_amd import ops, optim
from gated_gcrnns_amd.Modules import architectures as archit
from gated_gcrnns_amd.Utils import graphML

SWITCH, TAKE_ALL = 'GCRNN_NO_SMALL_CLS_GNN_HEAD', 'GCRNN_SMALL_CLS_GNN_HEAD'


def switched(fn, off):
    def run():
        if off:
            os.environ[SWITCH] = '1'
        else:
            os.environ.pop(SWITCH, None)
            os.environ[TAKE_ALL] = 'all'                     # also the rows that _small_cls_gnn_head_pays leaves to the two-module path
        try:
            return fn()
        finally:
            os.environ.pop(SWITCH, None)
            os.environ.pop(TAKE_ALL, None)
    return run


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--settle-ms', type=float, default=100.0)
    ap.add_argument('--batch', type=int, default=100)
    ap.add_argument('--steps', type=int, nargs='*', default=list(scb.STEPS))
    ap.add_argument('--dtypes', nargs='*', default=list(scb.DTYPES))
    ap.add_argument('--gatings', nargs='*', default=list(scb.GATINGS))
    ap.add_argument('--commit', default=None)
    ap.add_argument('--append', action='store_true', help='keep the lines already in --out')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'small_cls_gnn_head_bench.jsonl'))
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), 'small_cls_gnn_head_bench needs a ROCm device: a CPU timing says nothing about the GPU'
    dev = torch.device('cuda:0')
    rev = args.commit or scb.commit()
    has_new = hasattr(graphML.GGCRNNCell, 'classify_gnn')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    lines = []
    if args.append and os.path.exists(args.out):
        lines = [json.loads(ln) for ln in open(args.out) if ln.strip()]
    A = np.load(os.path.join(scb.GOLDEN, 'adj59.npy')).reshape(59, 59)
    S = A / np.max(np.abs(np.linalg.eigvals(A)))
    N, F, K, Ko, C, B = 59, 20, 4, 4, 11, args.batch
    for dname in args.dtypes:
        dt = scb.DTYPES[dname]
        for gname in args.gatings:
            tg, sg = scb.GATINGS[gname]
            torch.manual_seed(N + K)
            m = archit.GatedGCRNNforClassification(1, F, K, K, torch.tanh, torch.nn.ReLU, [C], S, True, tg, sg, torch.nn.ReLU, [F, 1], [Ko],
                                                   [N], graphML.NoPool, [1])      # examples/epicenter_estimation.py's GCRNNGNN
            m = m.to(dev).to(dt)
            opt = optim.make_trainer('ADAM', m.parameters(), 1e-3, 0.9, 0.999, flat=True)
            for T in args.steps:
                g = torch.Generator().manual_seed(T)
                x = torch.randn(B, T, 1, N, generator=g).to(dev, dt)
                h0 = torch.zeros(B, F, N, dtype=dt, device=dev)
                y = torch.randint(0, C, (B,), generator=g).to(dev)
                iters = args.iters if T < 200 else max(3, args.iters // 4)

                def infer():
                    with torch.no_grad():
                        return m(x, h0)

                def train():
                    opt.zero_grad()
                    loss = ops.cross_entropy(m(x, h0), y)
                    loss.backward()
                    opt.step()
                    ops.parameters_changed()
                    return loss

                for mode, fn in (('infer', infer), ('train', train)):
                    paths = {'off': switched(fn, True), 'new': switched(fn, False)}
                    line = dict(mode=mode, N=N, F=F, K=K, K_o=Ko, C=C, B=B, T=T, dtype=dname, gating=gname, reps=args.reps, iters=iters,
                                settle_ms=args.settle_ms, commit=rev, has_head_path=has_new)
                    times = {k: [] for k in paths}
                    for k, run in paths.items():
                        for _ in range(3):
                            run()
                        line[k + '_launches'], line[k + '_device_us'] = device_events(run)
                        line[k + '_peak_bytes'] = scb.peak_bytes(run)
                    for _ in range(args.reps):                       # interleaved
                        for k, run in paths.items():
                            times[k].append(scb.step_ms(run, iters, args.settle_ms))
                    for k, v in times.items():
                        line[k] = scb.summary(v)
                    line['ratio'] = round(line['off']['median_ms'] / line['new']['median_ms'], 3)
                    line['passes'] = bool(line['new']['median_ms'] <= line['off']['median_ms'] * (1 + line['off']['spread']))
                    lines.append(line)
                    print(json.dumps(line), flush=True)
                    with open(args.out, 'w') as fh:              # rewritten after every row: an interrupted run leaves what it measured
                        for done in lines:
                            fh.write(json.dumps(done) + '\n')
    return lines


if __name__ == '__main__':
    main()
