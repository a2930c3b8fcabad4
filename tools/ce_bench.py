#!/usr/bin/env python3
"""Loss + backward + accuracy of one classification step, on the one-pass HIP cross-entropy kernel (ops.cross_entropy: loss, gradient and
argmax hit count from one launch plus a fixed-order finish) against the composition the epicenter example used before it
(torch.nn.CrossEntropyLoss + backward, then argmax == labels, mean), per dtype and per (B, C) in {(100, 11), (256, 11), (8192, 64)}:
kernel launches per step (torch.profiler device events of one eager step) and host time per step, eager and as ONE captured graph.

    python tools/ce_bench.py [--reps 2000] [--warmup 200] [--settle-ms 100] [--out profiles/ce_bench.jsonl]

What is timed: a host clock around `reps` back-to-back steps that ends in a device synchronise, divided by reps. At the driver's sizes
(B = 100, C = 11) the work is microseconds and a step is launch-bound: this is the cost a training loop pays per step, not kernel time.
Both sides keep their results on the device (no host read inside a step): loss, d loss / d logits, and the accuracy as a 0-dim tensor.
Before each timed loop the device runs untimed steps for --settle-ms (the clock transient behind an idle period, as bench.py --settle-ms).
No threshold. The claims to support: "fewer launches" (a count) and "not slower under capture than the torch composition measured in the
same run". One JSON line per (dtype, B, C), with the commit the tree was at.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from gated_gcrnns_amd import ops

SHAPES = ((100, 11), (256, 11), (8192, 64))
DTYPES = {'f32': torch.float32, 'f64': torch.float64, 'bf16': torch.bfloat16}


def hip_step(z, lab):
    z.grad = None
    loss, hits = ops.cross_entropy(z, lab, return_hits=True)
    loss.backward()
    return loss, hits.to(loss.dtype) / z.shape[0]


def torch_step(z, lab):
    z.grad = None
    loss = torch.nn.functional.cross_entropy(z, lab)
    loss.backward()
    return loss, (z.detach().argmax(dim=1) == lab).to(torch.float64).mean()


def settle(fn, ms):
    t0 = time.perf_counter()
    while ms > 0 and 1e3 * (time.perf_counter() - t0) < ms:
        for _ in range(20):
            fn()
        torch.cuda.synchronize()


def per_call_us(fn, reps, warmup, settle_ms):
    settle(fn, settle_ms)
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / reps


def launches(fn):
    from torch.profiler import profile, ProfilerActivity
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def measure(step, z, lab, reps, warmup, settle_ms):
    fn = lambda: step(z, lab)
    for _ in range(3):
        fn()
    res = {'launches': launches(fn), 'eager_us': per_call_us(fn, reps, warmup, settle_ms)}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    z.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        fn()
    res['graph_us'] = per_call_us(graph.replay, reps, warmup, settle_ms)
    return res


def commit():
    try:
        return subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        return None


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=2000)
    ap.add_argument('--warmup', type=int, default=200)
    ap.add_argument('--settle-ms', type=float, default=100.0)
    ap.add_argument('--dtypes', default='f32,f64,bf16')
    ap.add_argument('--commit', default=None, help='recorded in every line (default: git rev-parse of the tree, null outside a checkout)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ce_bench.jsonl'))
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), 'ce_bench needs a ROCm device: a CPU timing says nothing about the GPU'
    dev = torch.device('cuda:0')
    rev = args.commit or commit()
    lines = []
    for dname in args.dtypes.split(','):
        for B, C in SHAPES:
            g = torch.Generator().manual_seed(B + C)
            z0 = (3.0 * torch.randn(B, C, generator=g)).to(dev, DTYPES[dname])
            lab = torch.randint(0, C, (B,), generator=g).to(dev)
            h = measure(hip_step, z0.clone().requires_grad_(True), lab, args.reps, args.warmup, args.settle_ms)
            t = measure(torch_step, z0.clone().requires_grad_(True), lab, args.reps, args.warmup, args.settle_ms)
            line = dict(dtype=dname, B=B, C=C, reps=args.reps, settle_ms=args.settle_ms, commit=rev,
                        hip_launches=h['launches'], torch_launches=t['launches'],
                        hip_eager_us=round(h['eager_us'], 2), torch_eager_us=round(t['eager_us'], 2),
                        hip_graph_us=round(h['graph_us'], 2), torch_graph_us=round(t['graph_us'], 2))
            lines.append(line)
            print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        for line in lines:
            fh.write(json.dumps(line) + '\n')
    return lines


if __name__ == '__main__':
    main()
