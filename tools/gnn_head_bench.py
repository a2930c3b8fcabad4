#!/usr/bin/env python3
"""Time the GNN output head (one graph-filter layer, ops.graph_filter_layer) against the composed filter path on the same shapes.

    python tools/gnn_head_bench.py [--B 256] [--T 32] [--N 1000] [--F 64] [--O 1] [--K 5] [--reps 20] [--out FILE]

Default: the flagship head -- all B*T = 8192 states of the SBM N = 1000 cell (bench.py's graph), 64 -> 1 features, K = 5,
bf16 H, fp32 weights, ReLU. Forward and backward (input + weight gradients) timed with HIP events after warm-up; the
composed path is GraphFilter.forward's LSIGF on fp32 (what the head ran on before the kernel). Prints one JSON line with the
times, the HBM floor from the bytes of H (+ y / dH) at 6.3 TB/s, and the speed-up.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

HBM_GBS = 6300.0


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=256)
    ap.add_argument('--T', type=int, default=32)
    ap.add_argument('--N', type=int, default=1000)
    ap.add_argument('--F', type=int, default=64)
    ap.add_argument('--O', type=int, default=1)
    ap.add_argument('--K', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--composed-reps', type=int, default=3)
    ap.add_argument('--no-composed', action='store_true', help='time the kernel only (counter runs)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from bench import sbm_graph
    from gated_gcrnns_amd import ops
    from gated_gcrnns_amd.graph import GraphOperator

    assert torch.cuda.is_available(), 'needs a ROCm device'
    dev = torch.device('cuda:0')
    items, N, F, O, K = args.B * args.T, args.N, args.F, args.O, args.K
    graph = GraphOperator(sbm_graph(N), device=dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    H = torch.randn((items, F, N), generator=gen, device=dev).to(torch.bfloat16).requires_grad_(True)
    w = (torch.randn((O, 1, K, F), generator=gen, device=dev) / (F * K) ** 0.5).requires_grad_(True)
    b = torch.zeros((O, 1), device=dev, requires_grad=True)
    dy = torch.randn((items, O, N), generator=gen, device=dev)
    assert ops.graph_filter_layer_supported(H.dtype, w.dtype, graph, F, O, K)

    y = ops.graph_filter_layer(H, w, b, graph, 'relu')
    fwd = timed(lambda: ops.graph_filter_layer(H.detach(), w.detach(), b.detach(), graph, 'relu'), args.reps)
    bwd = timed(lambda: torch.autograd.grad(y, (H, w, b), dy, retain_graph=True), args.reps)
    if args.no_composed:
        print(json.dumps(dict(head_forward_ms=fwd, head_backward_ms=bwd)))
        return
    with torch.no_grad():
        yc = ops._graph_filter_layer_composed(H, w, b, graph, 'relu')
        err = float((y.detach() - yc).abs().max()) / max(1.0, float(yc.abs().max()))
    del yc
    with torch.no_grad():
        cfwd = timed(lambda: ops._graph_filter_layer_composed(H, w, b, graph, 'relu'), args.composed_reps)
    yc = ops._graph_filter_layer_composed(H, w, b, graph, 'relu')
    cbwd = timed(lambda: torch.autograd.grad(yc, (H, w, b), dy, retain_graph=True), args.composed_reps)
    bytes_h = items * F * N * 2
    bytes_y = items * O * N * 4
    out = dict(shape=dict(B=args.B, T=args.T, N=N, F_in=F, F_out=O, K=K, nnz=graph.fwd[0].nnz, x='bf16', w='fp32', act='relu'),
               head_forward_ms=fwd, head_backward_ms=bwd, composed_forward_ms=cfwd, composed_backward_ms=cbwd,
               speedup_forward=cfwd / fwd, speedup_backward=cbwd / bwd,
               floor_forward_ms=(bytes_h + bytes_y) / HBM_GBS / 1e6, floor_backward_ms=(2 * bytes_h + 2 * bytes_y) / HBM_GBS / 1e6,
               achieved_forward_gbs=(bytes_h + bytes_y) / fwd / 1e6, achieved_backward_gbs=(2 * bytes_h + 2 * bytes_y) / bwd / 1e6,
               max_rel_diff_vs_composed=err)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
