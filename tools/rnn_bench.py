#!/usr/bin/env python3
"""Microseconds per call of the plain-RNN recurrence (the drivers' RNN baselines) at the envelope's shapes: the forward alone and a
training step (forward, L1 loss, backward), for the HIP kernels (ops.rnn_sequence), the composed step-by-step torch path and
torch.nn.RNN on the same device (a comparison only; the package does not use it). Medians over --reps timed calls after --warmup
untimed ones, each call timed by its own pair of device events. One JSON line per (shape, path).

    python tools/rnn_bench.py [--dtype f32|f64] [--reps 200] [--warmup 50]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from gated_gcrnns_amd import ops

SHAPES = [  # name, B, T, D, F_h
    ('kstep', 100, 5, 80, 1),
    ('quake_T20', 100, 20, 59, 21),
    ('quake_T200', 100, 200, 59, 21),
    ('large', 256, 32, 1000, 64),
]


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--dtype', default='f32', choices=['f32', 'f64'])
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--shapes', default=','.join(s[0] for s in SHAPES))
    args = ap.parse_args(argv)
    dt = torch.float32 if args.dtype == 'f32' else torch.float64
    dev = torch.device('cuda')
    out = []
    for name, B, T, D, Fh in SHAPES:
        if name not in args.shapes.split(','):
            continue
        torch.manual_seed(0)
        rnn = torch.nn.RNN(D, Fh, 1, nonlinearity='tanh', bias=True, batch_first=True).to(dev, dt)
        x = torch.randn(B, T, D, device=dev, dtype=dt)
        h0 = torch.zeros(B, Fh, device=dev, dtype=dt)
        y = torch.randn(B, T, Fh, device=dev, dtype=dt)
        params = [rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0]
        paths = {
            'kernel': lambda: ops.rnn_sequence(x, h0, *params, 'tanh'),
            'composed': lambda: ops._rnn_sequence_composed(x, h0, *params, 'tanh'),
            'torch.nn.RNN': lambda: rnn(x, h0.unsqueeze(0))[0],
        }
        for path, f in paths.items():
            def train():
                for p in params:
                    p.grad = None
                torch.nn.functional.l1_loss(f(), y).backward()
            with torch.no_grad():
                fwd = timed(f, args.reps, args.warmup)
            step = timed(train, args.reps, args.warmup)
            rec = dict(shape=name, B=B, T=T, D=D, F_h=Fh, dtype=args.dtype, path=path, forward_us=round(fwd, 2), train_step_us=round(step, 2))
            print(json.dumps(rec), flush=True)
            out.append(rec)
    return out


if __name__ == '__main__':
    main()
