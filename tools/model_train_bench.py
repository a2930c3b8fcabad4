#!/usr/bin/env python
"""One TRAINING step of the regression MODEL the k-step driver builds -- GatedGCRNNforRegression(64, 64, 5, 5, tanh, ReLU, [1], S, True,
time_gating=False|True, mlpType='multipMlp'): the cell plus one Linear(F -> 1) shared by all nodes -- on the bench's SBM graph (N = 1000),
B = 256, T = 32, bf16 inputs, fp32 master weights. A step is zero_grad, forward, batchTimeL1Loss on y, backward, FlatAdam. Public API only, so
the same file also runs on a checkout of an earlier commit:

    python tools/model_train_bench.py --tag this-tree  --out profiles/model_train_bench.jsonl
    (cd <checkout of the parent>; python <this file> --tag parent --root . --out <the same file>)
    GCRNN_NO_HEAD_CHAIN=1 python tools/model_train_bench.py --tag this-tree-two-modules --out ...      # the A/B switch, same binary

Method: host clock around `--steps` back-to-back steps (one synchronisation at the end) behind a settle phase of steps that lasts at least
`--settle-ms`, `--reps` repetitions; median / min / max per step, and the same interval by device events. torch.cuda.max_memory_allocated() is
reset before the timed steps and read behind them (the peak of a step; X, the target, the parameters and the optimiser state included). One
JSON line per model, printed and appended to --out. Only same-box, alternated runs compare."""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tag', default='tree')
    ap.add_argument('--root', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'), help='checkout to import the package and bench.sbm_graph from')
    ap.add_argument('--out', default=None)
    ap.add_argument('--B', type=int, default=256)
    ap.add_argument('--T', type=int, default=32)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--settle-ms', type=float, default=300.0)
    ap.add_argument('--round', type=int, default=0, help='label of an alternation round')
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    import torch
    from bench import sbm_graph
    import gated_gcrnns_amd.Modules.architectures as archit
    from gated_gcrnns_amd import ops
    from gated_gcrnns_amd.Utils.miscTools import batchTimeL1Loss
    from gated_gcrnns_amd.optim import FlatAdam

    dev = torch.device('cuda:0')
    N, F, G, K, B, T = 1000, 64, 64, 5, args.B, args.T
    S = sbm_graph(N)[0]
    rng = np.random.default_rng(3)
    X = torch.tensor(rng.standard_normal((B, T, G, N)), dtype=torch.float32, device=dev).to(torch.bfloat16)
    Y = torch.tensor(rng.standard_normal((B, T, 1, N)), dtype=torch.float32, device=dev).to(torch.bfloat16)
    h0 = torch.zeros((B, F, N), dtype=torch.bfloat16, device=dev)

    lines = []
    for tg in (False, True):
        torch.manual_seed(17)
        m = archit.GatedGCRNNforRegression(G, F, K, K, torch.tanh, torch.nn.ReLU, [1], S, True, time_gating=tg, spatial_gating=None,
                                           mlpType='multipMlp').to(dev).float()
        opt = FlatAdam(m.parameters(), lr=1e-4)
        last = {}

        def step():
            opt.zero_grad()
            loss = batchTimeL1Loss(m(X, h0), Y)
            loss.backward()
            opt.step()
            last['loss'] = loss

        step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < args.settle_ms:      # settle: the chip's clocks under this very load
            step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        host, devt = [], []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for _ in range(args.steps):
                step()
            e1.record()
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t0) * 1e3 / args.steps)
            devt.append(e0.elapsed_time(e1) / args.steps)
        peak = int(torch.cuda.max_memory_allocated(dev))
        lines.append({'tool': 'model_train_bench', 'tag': args.tag, 'round': args.round, 'head_chain_in_build': hasattr(ops, 'fused_cell_head_train'),
                      'time_gating': tg, 'B': B, 'T': T, 'N': N, 'F': F, 'G': G, 'K': K, 'steps': args.steps, 'reps': args.reps,
                      'host_ms_per_step': {'median': round(statistics.median(host), 4), 'min': round(min(host), 4), 'max': round(max(host), 4)},
                      'device_ms_per_step': {'median': round(statistics.median(devt), 4), 'min': round(min(devt), 4), 'max': round(max(devt), 4)},
                      'peak_allocated_bytes': peak, 'peak_allocated_GiB': round(peak / 2.0 ** 30, 4), 'loss': float(last['loss'].detach()),
                      'env': {k: v for k, v in os.environ.items() if k.startswith('GCRNN_')}})
        del m, opt
    for ln in lines:
        s = json.dumps(ln, sort_keys=True)
        print(s, flush=True)
        if args.out:
            with open(args.out, 'a') as fh:
                fh.write(s + '\n')


if __name__ == '__main__':
    main()
