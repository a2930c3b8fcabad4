#!/usr/bin/env python3
"""Generate the G15 golden vectors (GNN output heads) from the IMPORTED reference (build container only).

    python tests/golden/make_golden_gnn_heads.py          # needs the reference checkout (GCRNN_REFERENCE)

Same recipe as make_golden.py: the reference is imported read-only, run on CPU in float64, and only data is stored --
inputs, parameters by state_dict key, outputs and autograd gradients of a fixed linear loss sum(y * R):
  g15_sel_quake              the epicenter driver's 'Sel' (SelectionGNN F=[20, 21], K=[4], ReLU, NoPool, MLP [11]) on adj59
  g15_sel_kstep              the k-step driver's SelectionGNN([1, 8, 1], [10, 10], ReLU, NoPool) on the N = 50 SBM of G5
  g15_cls_gcrnngnn_{none,time}   the epicenter 'GCRNNGNN' (F_h = 20, K = 4, head [20, 1] K [4], MLP [11], final ReLU), T = 20
  g15_reg_gcrnngnn_{none,time}   regression, head [20, 1] K [5], no MLP, final ReLU, N = 50 SBM
  g15_reg_gcrnngnn_deep      regression, two-layer head [20, 4, 1] K [3, 2] (F_out > 1 and chaining)
  g15_trace_gcrnngnn         10 torch.optim.Adam steps of the epicenter GCRNNGNN on fixed batches: loss per step
"""
import os
import pickle
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

import make_golden as mg                   # noqa: E402  (imports the reference, float64 default)
from make_golden import archit, gml, sd_np, grads_np, save, sbm_gso, REF    # noqa: E402


def adj59():
    with open(os.path.join(REF, 'Adj.p'), 'rb') as f:
        A = np.asarray(pickle.load(f), dtype=np.float64)
    lam = np.max(np.abs(np.linalg.eigvals(A)))
    return (A / lam).reshape(1, 59, 59)


def run(m, inputs, R):
    """Forward, loss sum(y * R), backward; returns y, {param grads}, [input grads]."""
    ts = [torch.tensor(a, requires_grad=True) for a in inputs]
    y = m(*ts)
    (y * torch.tensor(R)).sum().backward()
    return y.detach().numpy(), grads_np(m), [t.grad.numpy().copy() for t in ts]


def g15_selection():
    rng = np.random.default_rng(150)
    S59 = adj59()
    torch.manual_seed(151)
    m = archit.SelectionGNN([20, 21], [4], True, torch.nn.ReLU, [59], gml.NoPool, [1], [11], S59[0])
    x = rng.standard_normal((6, 20, 59))
    R = rng.standard_normal((6, 11))
    p = sd_np(m)
    y, g, (gx,) = run(m, [x], R)
    save('g15_sel_quake', S=S59, x=x, R=R, y=y, params=p, grads=g, grad_x=gx, seed=np.array(151))
    S50, _ = sbm_gso(50, 5, 0.8, 0.2, 5)
    torch.manual_seed(152)
    m = archit.SelectionGNN([1, 8, 1], [10, 10], True, torch.nn.ReLU, [50, 50], gml.NoPool, [1, 1], [], S50[0])
    x = rng.standard_normal((7, 1, 50))
    R = rng.standard_normal((7, 50))
    p = sd_np(m)
    y, g, (gx,) = run(m, [x], R)
    save('g15_sel_kstep', S=S50, x=x, R=R, y=y, params=p, grads=g, grad_x=gx, seed=np.array(152))


def g15_gcrnn_heads():
    rng = np.random.default_rng(153)
    S59 = adj59()
    B, T = 4, 20
    x = rng.standard_normal((B, T, 1, 59))
    h0 = 0.3 * rng.standard_normal((B, 20, 59))
    R = rng.standard_normal((B, 11))
    for name, tg in (('none', False), ('time', True)):
        torch.manual_seed(154)
        m = archit.GatedGCRNNforClassification(1, 20, 4, 4, torch.tanh, torch.nn.ReLU, [11], S59[0], True, tg, None,
                                               finalNonlinearity=torch.nn.ReLU, dimNodeSignals=[20, 1], nFilterTaps=[4],
                                               nSelectedNodes=[59], poolingFunction=gml.NoPool, poolingSize=[1])
        p = sd_np(m)
        y, g, (gx, gh0) = run(m, [x, h0], R)
        save('g15_cls_gcrnngnn_' + name, S=S59, x=x, h0=h0, R=R, y=y, params=p, grads=g, grad_x=gx, grad_h0=gh0, seed=np.array(154))
    S50, _ = sbm_gso(50, 5, 0.8, 0.2, 5)
    B, T = 3, 6
    x = rng.standard_normal((B, T, 1, 50))
    h0 = 0.3 * rng.standard_normal((B, 20, 50))
    R = rng.standard_normal((B, T, 1, 50))
    for name, tg, F, K in (('none', False, [20, 1], [5]), ('time', True, [20, 1], [5]), ('deep', False, [20, 4, 1], [3, 2])):
        torch.manual_seed(155)
        m = archit.GatedGCRNNforRegression(1, 20, 2, 2, torch.tanh, torch.nn.ReLU, [], S50[0], True, tg, None, 'oneMlp',
                                           torch.nn.ReLU, F, K, [50] * len(K), gml.NoPool, [1] * len(K))
        p = sd_np(m)
        y, g, (gx, gh0) = run(m, [x, h0], R)
        save('g15_reg_gcrnngnn_' + name, S=S50, x=x, h0=h0, R=R, y=y, params=p, grads=g, grad_x=gx, grad_h0=gh0,
             F=np.array(F), K=np.array(K), seed=np.array(155))


def g15_trace():
    rng = np.random.default_rng(156)
    S59 = adj59()
    B, T, steps = 4, 20, 10
    x = rng.standard_normal((steps, B, T, 1, 59))
    labels = rng.integers(0, 11, (steps, B))
    h0 = np.zeros((B, 20, 59))
    torch.manual_seed(157)
    m = archit.GatedGCRNNforClassification(1, 20, 4, 4, torch.tanh, torch.nn.ReLU, [11], S59[0], True, False, None,
                                           finalNonlinearity=torch.nn.ReLU, dimNodeSignals=[20, 1], nFilterTaps=[4],
                                           nSelectedNodes=[59], poolingFunction=gml.NoPool, poolingSize=[1])
    p0 = sd_np(m)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, betas=(0.9, 0.999))
    loss_fn = torch.nn.CrossEntropyLoss()
    losses = []
    for it in range(steps):
        m.zero_grad()
        loss = loss_fn(m(torch.tensor(x[it]), torch.tensor(h0)), torch.tensor(labels[it]))
        loss.backward()
        opt.step()
        losses.append(loss.item())
    save('g15_trace_gcrnngnn', S=S59, x=x, labels=labels, h0=h0, params0=p0, params10=sd_np(m), loss=np.array(losses))


if __name__ == '__main__':
    assert mg.TOL > 0
    g15_selection()
    g15_gcrnn_heads()
    g15_trace()
