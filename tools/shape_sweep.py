#!/usr/bin/env python3
"""Robustness sweep of the GGCRNNCell dispatch on the GPU box: every gating x {inference, training} x batch sizes / channel counts / step counts /
graph weightings at N = 1000 (sparse SBM), each run once on the default dispatch and once with the wide kernel and the inline layouts switched off
(GCRNN_SEQ32=0 GCRNN_NO_INLINE_PACK=1): no exception, finite results, and the two within bf16 noise of each other.
python3 tools/shape_sweep.py [quick] [axes | f32 | large]"""
import itertools
import os
import sys
import traceback
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
import gated_gcrnns_amd.Utils.graphML as gml


def random_graph(N, seed=3):
    rng = np.random.default_rng(seed)
    W = (rng.random((N, N)) < min(1.0, 10.0 / N)).astype(np.float64)
    W = np.triu(W, 1)
    W = W + W.T
    return (W / np.max(np.abs(np.linalg.eigvalsh(W)))).reshape(1, N, N)


def pin_cell_to_torch_reference(cell64, S, X, h0, H64, items=2):
    """The fp64 cell a sweep takes as its truth against the plain-torch fp64 reference (oracle/torch_reference.py: dense S, torch's own ops)
    on the first `items` sequences: states within 1e-11."""
    from oracle import torch_reference as tr
    p = {k: v.detach().double() for k, v in cell64.state_dict().items()}
    Sd = torch.as_tensor(np.asarray(S), dtype=torch.float64).to(X.device)
    with torch.no_grad():
        Hr = tr.ggcrnn_cell(p, Sd.reshape(-1, Sd.shape[-1], Sd.shape[-1]), X[:items].double(), h0[:items].double(),
                            cell64.time_gating == True, cell64.spatial_gating)  # noqa: E712
    d = float((H64[:items].double() - Hr).abs().max())
    assert d <= 1e-11, 'the fp64 cell differs from the torch reference: %.3g' % d


def sweep_f32(dev, quick=False, N=1000, Bs=None):
    """fp32 cells (the x3 kernels where they apply, else the composed path) against the fp64 composed path on the same parameters and inputs:
    H within 2e-5, every gradient within 3e-4 of its max (edge gates: 6e-3; scalars 5e-3)."""
    import copy
    K = 5
    fails, n = [], 0
    pinned = set()
    gatings = ((False, None), (True, None), (False, 'node'), (True, 'node'), (False, 'edge'))
    for gname in ('uniform', 'normalized'):
        if N == 1000:
            St = torch.tensor(bench.sbm_graph(N, normalized=(gname == 'normalized')))
        else:      # (other sizes, e.g. beyond the LDS-resident kernels' 1024 nodes: a random graph; "normalized" = D^-1/2 W D^-1/2 scaled by its lambda_max)
            Wn = random_graph(N)[0]
            if gname == 'normalized':
                dg = np.maximum((Wn != 0).sum(axis=1), 1).astype(np.float64)
                Wn = (Wn != 0) / np.sqrt(np.outer(dg, dg))
                Wn = Wn / np.max(np.abs(np.linalg.eigvalsh(Wn)))
            St = torch.tensor(Wn.reshape(1, N, N))
        for (tg, sg), F, G, B, train in itertools.product(gatings, (64,) if quick else (32, 64), (1, 64), Bs or ((100,) if quick else (100, 256)), (False, True)):
            if sg == 'edge' and (gname == 'normalized' or B > 128):
                continue
            T = 3
            tag = 'f32 N=%d %s tg=%s sg=%s F=%d G=%d T=%d B=%d %s' % (N, gname, tg, sg, F, G, T, B, 'train' if train else 'infer')
            n += 1
            try:
                torch.manual_seed(2)
                cell = gml.GGCRNNCell(G, F, K, K, torch.tanh, tg, sg, 1, True)
                cell.addGSO(St)
                cell = cell.float().to(dev)
                ref = copy.deepcopy(cell).double()
                X = torch.randn(B, T, G, N, device=dev)
                h0 = 0.3 * torch.randn(B, F, N, device=dev) if (B % 2) else torch.zeros(B, F, N, device=dev)
                tgt = torch.randn(B, T, F, N, device=dev)

                def run(c, X, h0, tgt):
                    if not train:
                        with torch.no_grad():
                            return c(X, h0).double(), {}
                    for q in c.parameters():
                        q.grad = None
                    H = c(X, h0)
                    (H * tgt).sum().backward()
                    return H.detach().double(), {k: q.grad.detach().double().clone() for k, q in c.named_parameters() if q.grad is not None}
                H1, g1 = run(cell, X, h0, tgt)
                Hr, gr = run(ref, X.double(), h0.double(), tgt.double())
                if (gname, tg, sg, train) not in pinned:           # the truth itself, once per graph, gating and mode
                    pinned.add((gname, tg, sg, train))
                    pin_cell_to_torch_reference(ref, St, X, h0, Hr)
                d = float((H1 - Hr).abs().max())
                assert d <= 2e-5, 'H differs from fp64: %.3g' % d
                assert g1.keys() == gr.keys(), 'gradient sets differ'
                gmax = max([float(v.abs().max()) for v in gr.values()] + [0.0])
                for k in gr:
                    sc = max(float(gr[k].abs().max()), 1e-3 * gmax)      # (a parameter whose gradient is tiny beside the others': absolute noise)
                    dd = float((g1[k] - gr[k]).abs().max())
                    tol = 5e-3 if g1[k].numel() == 1 else (6e-3 if sg == 'edge' else 3e-4)      # (fp32 sums over B T N (x edges) terms, the attention's LeakyReLU kinks; a scalar's own size is no scale for its noise)
                    assert dd <= tol * max(sc, 1e-2), 'grad %s differs: %.3g of %.3g' % (k, dd, sc)
            except Exception as e:      # noqa: BLE001
                fails.append((tag, repr(e)[:300]))
                print('FAIL', tag, repr(e)[:300], flush=True)
                if os.environ.get('SWEEP_TRACE'):
                    traceback.print_exc()
    print('shape sweep (f32 vs fp64, N = %d): %d combinations, %d failures' % (N, n, len(fails)))
    for t, e in fails:
        print('  ', t, e)
    return n, fails


def sweep_bf16_large(dev, Ns=(1500, 2048)):
    """bf16 cells on graphs beyond the LDS-resident kernels (streaming / composed path), every gating, against the same cell in fp64:
    H within 6e-2, the gradient vector within 10 % in the L2 norm."""
    import copy
    K, B, T = 5, 20, 3
    fails, n = [], 0
    for N in Ns:
        S = torch.tensor(random_graph(N, seed=4))
        for (tg, sg), (F, G), train in itertools.product(((False, None), (True, None), (False, 'node'), (True, 'node'), (False, 'edge')),
                                                         ((64, 64), (20, 1), (32, 32)), (False, True)):
            tag = 'bf16 N=%d tg=%s sg=%s F=%d G=%d %s' % (N, tg, sg, F, G, 'train' if train else 'infer')
            n += 1
            try:
                torch.manual_seed(2)
                c = gml.GGCRNNCell(G, F, K, K, torch.tanh, tg, sg, 1, True)
                c.addGSO(S)
                with torch.no_grad():
                    c.weight_A.mul_(0.25 if G == 1 else 1.0)
                c = c.to(torch.bfloat16).to(dev)
                r = copy.deepcopy(c).double()
                X = torch.randn(B, T, G, N, device=dev).to(torch.bfloat16)
                h0 = (0.3 * torch.randn(B, F, N, device=dev)).to(torch.bfloat16)
                if train:
                    H = c(X, h0)
                    H.float().sum().backward()
                    Hr = r(X.double(), h0.double())
                    Hr.sum().backward()
                    num = sum(float(((p.grad.double() - q.grad) ** 2).sum()) for p, q in zip(c.parameters(), r.parameters()) if q.grad is not None) ** 0.5
                    den = sum(float((q.grad ** 2).sum()) for q in r.parameters() if q.grad is not None) ** 0.5
                    assert num <= 0.1 * den, 'gradient differs: %.3g of %.3g (L2)' % (num, den)
                else:
                    with torch.no_grad():
                        H, Hr = c(X, h0), r(X.double(), h0.double())
                d = float((H.double() - Hr).abs().max())
                assert d <= 6e-2, 'H differs: %.3g' % d
            except Exception as e:      # noqa: BLE001
                fails.append((tag, repr(e)[:300]))
                print('FAIL', tag, repr(e)[:300], flush=True)
                if os.environ.get('SWEEP_TRACE'):
                    traceback.print_exc()
    print('shape sweep (bf16 vs fp64, N = %s): %d combinations, %d failures' % ('/'.join(str(x) for x in Ns), n, len(fails)))
    return n, fails


def main(quick=False, axes=False):
    """axes: the other axes -- K in {2, 3, 4}, N in {104, 400, 999, 1024} (999: rows that are not 16-byte multiples), uniform-weight graphs."""
    dev = torch.device('cuda:0')
    N, K = 1000, 5
    graphs = {'uniform': bench.sbm_graph(N), 'normalized': bench.sbm_graph(N, normalized=True)}
    Bs = (100, 256) if quick else (3, 64, 100, 128, 160, 256)
    Gs = (1, 64) if quick else (1, 32, 64)
    Fs = (64,) if quick else (32, 64)
    Ts = (4,) if quick else (1, 5)
    if axes:
        fails, n = [], 0
        for Nn in ((999,) if quick else (104, 400, 999, 1024)):
            S1 = random_graph(Nn)
            for Kk in ((3,) if quick else (2, 3, 4)):
                n1, f1 = sweep({'uniform N=%d K=%d' % (Nn, Kk): S1}, Nn, Kk, (100, 256), (1, 64), (32, 64), (3,), dev)
                n += n1
                fails += f1
        print('shape sweep (axes): %d combinations, %d failures' % (n, len(fails)))
        for t, e in fails:
            print('  ', t, e)
        return n, fails
    n, fails = sweep(graphs, N, K, Bs, Gs, Fs, Ts, dev)
    print('shape sweep: %d combinations, %d failures' % (n, len(fails)))
    for t, e in fails:
        print('  ', t, e)
    return n, fails


def sweep(graphs, N, K, Bs, Gs, Fs, Ts, dev):
    gatings = ((False, None), (True, None), (False, 'node'), (True, 'node'), (False, 'edge'))
    SWITCHES = {'GCRNN_SEQ32': '0', 'GCRNN_NO_INLINE_PACK': '1'}
    fails, n = [], 0
    for gname, S in graphs.items():
        St = torch.tensor(S)
        for (tg, sg), F, G, T, B, train in itertools.product(gatings, Fs, Gs, Ts, Bs, (False, True)):
            if sg == 'edge' and (gname == 'normalized' or B > 128):      # (edge gates: the attention path is per edge, keep the sweep short)
                continue
            tag = '%s tg=%s sg=%s F=%d G=%d T=%d B=%d %s' % (gname, tg, sg, F, G, T, B, 'train' if train else 'infer')
            n += 1
            try:
                torch.manual_seed(1)
                cell = gml.GGCRNNCell(G, F, K, K, torch.tanh, tg, sg, 1, True)
                cell.addGSO(St)
                cell = cell.to(torch.bfloat16).to(dev)
                X = torch.randn(B, T, G, N, device=dev).to(torch.bfloat16)
                h0 = (0.3 * torch.randn(B, F, N, device=dev)).to(torch.bfloat16) if (B % 2) else torch.zeros(B, F, N, dtype=torch.bfloat16, device=dev)
                tgt = torch.randn(B, T, F, N, device=dev).to(torch.bfloat16)

                def run():
                    if not train:
                        with torch.no_grad():
                            return cell(X, h0).float(), {}
                    for q in cell.parameters():
                        q.grad = None
                    H = cell(X, h0)
                    (H.float() * tgt.float()).sum().backward()
                    return H.detach().float(), {k: q.grad.detach().float().clone() for k, q in cell.named_parameters() if q.grad is not None}
                H1, g1 = run()
                old = {k: os.environ.get(k) for k in SWITCHES}
                os.environ.update(SWITCHES)
                for k in ('_fused_plan_rank1', '_fused_plan_rank1_adj'):
                    cell.graph.__dict__.pop(k, None)
                try:
                    H0, g0 = run()
                finally:
                    for k, v in old.items():
                        if v is None:
                            os.environ.pop(k, None)
                        else:
                            os.environ[k] = v
                assert torch.isfinite(H1).all() and torch.isfinite(H0).all(), 'non-finite state'
                d = (H1 - H0).abs()
                # (one input feature: input taps of size 1 / sqrt(K) drive the states into a regime where a step amplifies bf16 noise ~2x -- both kernel
                #  families sit 0.02-0.09 from the fp64 result by T = 5, tools/sweep_case.py; the wide kernel rounds w^k W_k where the others keep bf16 parameters exact)
                hmax = 0.2 if G == 1 else 6e-2
                assert float(d.max()) <= hmax and float(d.mean()) <= 3e-3, 'H differs: max %.3g mean %.3g' % (float(d.max()), float(d.mean()))
                assert g1.keys() == g0.keys(), 'gradient sets differ'
                smax = max([float(v.abs().max()) for v in g0.values() if v.numel() == 1] + [0.0])
                for k in g1:
                    sc = float(g0[k].abs().max())
                    dd = float((g1[k] - g0[k]).abs().max())
                    tol = 0.4 if g1[k].numel() == 1 else 8e-2      # (a scalar's gradient is one sum with cancellation: its own size is no scale for its noise --
                    if g1[k].numel() == 1:                          #  GFL_node_in.0.bias = 0.54 beside its sibling's 463 at tg + node, G = 1, B = 64: both kernel families
                        sc = max(sc, 0.02 * smax)                   #  sit 0.5-0.9 from the fp64 value, tools/sweep_case.py -- so the cell's largest scalar gradient bounds the scale from below)
                    assert torch.isfinite(g1[k]).all() and dd <= tol * max(sc, 1e-6), 'grad %s differs: %.3g of %.3g' % (k, dd, sc)
            except Exception as e:      # noqa: BLE001
                fails.append((tag, repr(e)[:300]))
                print('FAIL', tag, repr(e)[:300], flush=True)
                if os.environ.get('SWEEP_TRACE'):
                    traceback.print_exc()
            if n % 50 == 0:
                print('%d combinations, %d failures' % (n, len(fails)), flush=True)
    return n, fails


if __name__ == '__main__':
    if 'f32' in sys.argv[1:]:
        sys.exit(1 if sweep_f32(torch.device('cuda:0'), 'quick' in sys.argv[1:])[1] else 0)
    if 'large' in sys.argv[1:]:      # graphs beyond the LDS-resident kernels (streaming / composed path)
        bad = sweep_f32(torch.device('cuda:0'), False, 1500, (20,))[1] + sweep_f32(torch.device('cuda:0'), False, 2048, (20,))[1] + sweep_bf16_large(torch.device('cuda:0'))[1]
        sys.exit(1 if bad else 0)
    sys.exit(1 if main('quick' in sys.argv[1:], 'axes' in sys.argv[1:])[1] else 0)
