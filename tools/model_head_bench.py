#!/usr/bin/env python
"""Inference forward of the regression MODEL the k-step driver builds -- GatedGCRNNforRegression(64, 64, 5, 5, tanh, ReLU, [1], S, True,
time_gating=False|True, mlpType='multipMlp'): the cell plus one Linear(F -> 1) shared by all nodes -- on the bench's SBM graph (N = 1000),
B = 256, T = 32, bf16, under no_grad. Public API only, so the same file also runs on a checkout of an earlier commit:

    python tools/model_head_bench.py --tag this-tree  --out profiles/model_head_bench.jsonl
    (cd <checkout of the parent>; python <this file> --tag parent --root . --out <the same file>)

Method: host clock around `--fwds` back-to-back forwards (one synchronisation at the end) behind a settle phase of forwards that lasts at least
`--settle-ms`, `--reps` repetitions; median / min / max per forward, and the same interval by device events. One JSON line per point, printed and
appended to --out. Also the same build's cell-alone forward (H in the user layout; for information). Only same-box, alternated runs compare."""
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
    ap.add_argument('--fwds', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--settle-ms', type=float, default=100.0)
    ap.add_argument('--round', type=int, default=0, help='label of an alternation round')
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    import torch
    from bench import sbm_graph
    import gated_gcrnns_amd.Modules.architectures as archit
    from gated_gcrnns_amd import ops

    dev = torch.device('cuda:0')
    N, F, G, K, B, T = 1000, 64, 64, 5, args.B, args.T
    S = sbm_graph(N)[0]
    rng = np.random.default_rng(3)
    X = torch.tensor(rng.standard_normal((B, T, G, N)), dtype=torch.float32, device=dev).to(torch.bfloat16)
    h0 = torch.zeros((B, F, N), dtype=torch.bfloat16, device=dev)

    def measure(fn):
        with torch.no_grad():
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            while (time.perf_counter() - t0) * 1e3 < args.settle_ms:      # settle: the chip's clocks under this very load
                fn()
            host, devt = [], []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                for _ in range(args.fwds):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                host.append((time.perf_counter() - t0) * 1e3 / args.fwds)
                devt.append(e0.elapsed_time(e1) / args.fwds)
        return host, devt

    lines = []
    for tg in (False, True):
        torch.manual_seed(17)
        m = archit.GatedGCRNNforRegression(G, F, K, K, torch.tanh, torch.nn.ReLU, [1], S, True, time_gating=tg, spatial_gating=None,
                                           mlpType='multipMlp').to(dev).to(torch.bfloat16)
        for what, fn in (('model', lambda: m(X, h0)), ('cell_alone', lambda: m.stateGCRNN(X, h0))):
            host, devt = measure(fn)
            lines.append({'tool': 'model_head_bench', 'tag': args.tag, 'round': args.round, 'what': what, 'wide_head_in_build': hasattr(ops, 'fused_cell_forward_wide_head'), 'time_gating': tg, 'B': B, 'T': T, 'N': N, 'F': F, 'G': G,
                          'K': K, 'fwds': args.fwds, 'reps': args.reps,
                          'host_ms_per_forward': {'median': round(statistics.median(host), 4), 'min': round(min(host), 4), 'max': round(max(host), 4)},
                          'device_ms_per_forward': {'median': round(statistics.median(devt), 4), 'min': round(min(devt), 4), 'max': round(max(devt), 4)},
                          'us_per_step_median': round(1e3 * statistics.median(host) / T, 2),
                          'env': {k: v for k, v in os.environ.items() if k.startswith('GCRNN_')}})
    for ln in lines:
        s = json.dumps(ln, sort_keys=True)
        print(s, flush=True)
        if args.out:
            with open(args.out, 'a') as fh:
                fh.write(s + '\n')


if __name__ == '__main__':
    main()
