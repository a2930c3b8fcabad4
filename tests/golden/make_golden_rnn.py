#!/usr/bin/env python3
"""Generate the G16 golden vectors (the drivers' plain-RNN baselines) from the IMPORTED reference (build container only).

    python tests/golden/make_golden_rnn.py          # needs the reference checkout (GCRNN_REFERENCE)

Same recipe as make_golden.py: the reference is imported read-only, run on CPU in float64, and only data is stored --
inputs, parameters by state_dict key, outputs and autograd gradients of a fixed linear loss sum(y * R):
  g16_rnn_reg_kstep    the k-step driver's 'RNNMLP': RNNforRegression(1, 1, 'tanh', [1], ReLU), N = 80 (D = 80, F_h = 1), T = 5
  g16_rnn_cls_quake    the epicenter driver's 'RNNMLP': RNNforClassification(1, 21, 'tanh', [11], ReLU) on adj59, T = 20
  g16_rnn_reg_deep     RNNforRegression(2, 8, 'relu', [6, 1], ReLU, bias=False, final ReLU), N = 30 (D = 60: the f*N + n order)
  g16_trace_rnnmlp     10 torch.optim.Adam steps of the k-step RNNMLP on fixed batches (L1 loss): loss per step
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

import make_golden as mg                   # noqa: E402  (imports the reference, float64 default)
from make_golden import archit, sd_np, grads_np, save, sbm_gso    # noqa: E402
from make_golden_gnn_heads import adj59    # noqa: E402


def g16_models():
    rng = np.random.default_rng(160)
    S80, _ = sbm_gso(80, 5, 0.8, 0.2, 6)
    B, T = 4, 5
    torch.manual_seed(161)
    m = archit.RNNforRegression(1, 1, 'tanh', [1], torch.nn.ReLU, S80[0], True)
    x = rng.standard_normal((B, T, 1, 80))
    h0 = 0.3 * rng.standard_normal((B, 1))
    R = rng.standard_normal((B, T, 1, 80))
    p = sd_np(m)
    y, g, gx, gh0 = run_rnn(m, x, h0, R)
    save('g16_rnn_reg_kstep', S=S80, x=x, h0=h0, R=R, y=y, params=p, grads=g, grad_x=gx, grad_h0=gh0, seed=np.array(161))

    S59 = adj59()
    B, T = 4, 20
    torch.manual_seed(162)
    m = archit.RNNforClassification(1, 21, 'tanh', [11], torch.nn.ReLU, S59[0], True)
    x = rng.standard_normal((B, T, 1, 59))
    h0 = 0.3 * rng.standard_normal((B, 21))
    R = rng.standard_normal((B, 11))
    p = sd_np(m)
    y, g, gx, gh0 = run_rnn(m, x, h0, R)
    save('g16_rnn_cls_quake', S=S59, x=x, h0=h0, R=R, y=y, params=p, grads=g, grad_x=gx, grad_h0=gh0, seed=np.array(162))

    S30, _ = sbm_gso(30, 3, 0.8, 0.2, 7)
    B, T = 3, 6
    torch.manual_seed(163)
    m = archit.RNNforRegression(2, 8, 'relu', [6, 1], torch.nn.ReLU, S30[0], False, finalNonlinearity=torch.nn.ReLU)
    x = rng.standard_normal((B, T, 2, 30))
    h0 = 0.3 * rng.standard_normal((B, 8))
    R = rng.standard_normal((B, T, 1, 30))
    p = sd_np(m)
    y, g, gx, gh0 = run_rnn(m, x, h0, R)
    save('g16_rnn_reg_deep', S=S30, x=x, h0=h0, R=R, y=y, params=p, grads=g, grad_x=gx, grad_h0=gh0, seed=np.array(163))


def run_rnn(m, x, h0, R):
    """Forward archit(x, h0, c0 = h0), loss sum(y * R), backward; returns y, {param grads}, grad x, grad h0."""
    xt = torch.tensor(x, requires_grad=True)
    ht = torch.tensor(h0, requires_grad=True)
    y = m(xt, ht, ht)
    (y * torch.tensor(R)).sum().backward()
    return y.detach().numpy(), grads_np(m), xt.grad.numpy().copy(), ht.grad.numpy().copy()


def g16_trace():
    rng = np.random.default_rng(164)
    S80, _ = sbm_gso(80, 5, 0.8, 0.2, 6)
    B, T, steps = 4, 5, 10
    x = rng.standard_normal((steps, B, T, 1, 80))
    yb = rng.standard_normal((steps, B, T, 1, 80))
    torch.manual_seed(165)
    m = archit.RNNforRegression(1, 1, 'tanh', [1], torch.nn.ReLU, S80[0], True)
    p0 = sd_np(m)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, betas=(0.9, 0.999))
    loss_fn = torch.nn.L1Loss()
    losses = []
    for it in range(steps):
        m.zero_grad()
        h0 = torch.zeros(B, 1)
        loss = loss_fn(m(torch.tensor(x[it]), h0, h0), torch.tensor(yb[it]))
        loss.backward()
        opt.step()
        losses.append(loss.item())
    save('g16_trace_rnnmlp', S=S80, x=x, y=yb, params0=p0, params10=sd_np(m), loss=np.array(losses), seed=np.array(165))


if __name__ == '__main__':
    assert mg.TOL > 0
    g16_models()
    g16_trace()
