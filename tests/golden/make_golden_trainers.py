#!/usr/bin/env python3
"""Generate the G17 golden vectors (the drivers' SGD / RMSprop trainers and learning-rate decay) from the IMPORTED reference
(build container only).

    python tests/golden/make_golden_trainers.py          # needs the reference checkout (GCRNN_REFERENCE)

Same recipe and helpers as make_golden.py's g6_training_trace: the reference is imported read-only, run on CPU in float64, and only
arrays are stored -- graph, x, y, params0, per-step loss and metric, final parameters, the hyper-parameters, and for the decay traces
the learning rate in force at every step:
  g17_trace_sgd, g17_trace_rmsprop       20 steps of G6's GCRNNMLP (same graph, data and seed) under torch.optim.SGD(lr) and
                                         torch.optim.RMSprop(lr, alpha=0.9) as the driver constructs them (kStepPredGRNNs.py:710-714).
                                         lr is chosen so that the loss visibly moves over 20 steps and is recorded in the file.
  g17_trace_adam_decay_p1 / _p2          3 epochs x 4 fixed batches of 5 (batch order = sample order) of the same model under Adam(1e-3)
                                         + StepLR(period 1 / 2, rate 0.9) stepped at the TOP of each epoch as the reference does
                                         (Modules/train_rnn.py:197-200): with period 1 the first epoch already trains at 0.9e-3.
  g17_trace_rnnmlp_rmsprop_decay         the k-step driver's RNNMLP (G16's model and graph), 3 epochs x 2 batches of 4 under
                                         RMSprop(1e-2, alpha=0.9) + StepLR(period 2, rate 0.5): the non-GCRNN branch of MultipleModels.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

import make_golden as mg                                   # noqa: E402  (imports the reference, float64 default)
from make_golden import archit, misc, sd_np, save, sbm_gso  # noqa: E402

SGD_LR, RMSPROP_LR, RMSPROP_ALPHA = 0.02, 1e-3, 0.9


def g6_data():
    """Graph and data of g6_training_trace (make_golden.py), drawn by the same recipe and seeds."""
    S, W = sbm_gso(50, 5, 0.8, 0.2, 6)
    rng = np.random.default_rng(16)
    B, T, N = 20, 5, 50
    A = S[0]
    xs = np.zeros((B, T + 1, N))
    xs[:, 0] = rng.random((B, N))
    for t in range(T):
        xs[:, t + 1] = xs[:, t] @ A + 0.1 * rng.standard_normal((B, N))
    return S, xs[:, :T].reshape(B, T, 1, N), xs[:, 1:].reshape(B, T, 1, N)


def g6_model(A):
    torch.manual_seed(60)
    return archit.GatedGCRNNforRegression(1, 20, 3, 3, torch.tanh, torch.nn.ReLU, [1], A, True,
                                          time_gating=False, spatial_gating=None, mlpType='multipMlp')


def step(m, opt, x, y, h0, loss_fn):
    m.zero_grad()
    yhat = m(torch.tensor(x), *h0)
    loss = loss_fn(yhat, torch.tensor(y))
    loss.backward()
    opt.step()
    return loss.item(), misc.batchTimeMSELoss(yhat.detach(), torch.tensor(y)).item()


def g17_plain():
    S, x, y = g6_data()
    h0 = (torch.zeros(x.shape[0], 20, x.shape[3]),)
    for tag, make, hyper in (('sgd', lambda p: torch.optim.SGD(p, lr=SGD_LR), dict(lr=SGD_LR)),
                             ('rmsprop', lambda p: torch.optim.RMSprop(p, lr=RMSPROP_LR, alpha=RMSPROP_ALPHA),
                              dict(lr=RMSPROP_LR, alpha=RMSPROP_ALPHA))):
        m = g6_model(S[0])
        p0 = sd_np(m)
        opt = make(m.parameters())
        trace = [step(m, opt, x, y, h0, misc.batchTimeL1Loss) for _ in range(20)]
        loss, metric = np.array(trace).T
        print('g17_trace_%s: loss %.6f -> %.6f' % (tag, loss[0], loss[-1]))
        save('g17_trace_' + tag, S=S, x=x, y=y, params0=p0, params20=sd_np(m), loss=loss, metric=metric,
             **{k: np.array(v) for k, v in hyper.items()})


def decay_trace(m, opt, x, y, h0_of, loss_fn, nEpochs, batch, period, rate):
    """The reference's loop (Modules/train_rnn.py:149-155, 191-276) without the permutation: StepLR stepped at the top of each epoch."""
    sched = torch.optim.lr_scheduler.StepLR(opt, period, rate)
    loss, metric, lrs = [], [], []
    for epoch in range(nEpochs):
        sched.step()
        for b in range(0, x.shape[0], batch):
            lrs.append(opt.param_groups[0]['lr'])
            lo, me = step(m, opt, x[b:b + batch], y[b:b + batch], h0_of(batch), loss_fn)
            loss.append(lo)
            metric.append(me)
    return np.array(loss), np.array(metric), np.array(lrs)


def g17_adam_decay():
    S, x, y = g6_data()
    for period in (1, 2):
        m = g6_model(S[0])
        p0 = sd_np(m)
        opt = torch.optim.Adam(m.parameters(), lr=1e-3, betas=(0.9, 0.999))
        loss, metric, lrs = decay_trace(m, opt, x, y, lambda B: (torch.zeros(B, 20, x.shape[3]),), misc.batchTimeL1Loss, 3, 5, period, 0.9)
        print('g17_trace_adam_decay_p%d: lr' % period, sorted(set(lrs.tolist()), reverse=True))
        save('g17_trace_adam_decay_p%d' % period, S=S, x=x, y=y, params0=p0, params_final=sd_np(m), loss=loss, metric=metric, lr=lrs,
             lr0=np.array(1e-3), period=np.array(period), rate=np.array(0.9), epochs=np.array(3), batch=np.array(5))


def g17_rnnmlp():
    rng = np.random.default_rng(170)
    S80, _ = sbm_gso(80, 5, 0.8, 0.2, 6)
    n, T = 8, 5
    x = rng.standard_normal((n, T, 1, 80))
    y = rng.standard_normal((n, T, 1, 80))
    torch.manual_seed(171)
    m = archit.RNNforRegression(1, 1, 'tanh', [1], torch.nn.ReLU, S80[0], True)
    p0 = sd_np(m)
    opt = torch.optim.RMSprop(m.parameters(), lr=1e-2, alpha=0.9)
    h0_of = lambda B: (torch.zeros(B, 1), torch.zeros(B, 1))                          # c0 = h0 (reference train_rnn.py:248-250)
    loss, metric, lrs = decay_trace(m, opt, x, y, h0_of, misc.batchTimeL1Loss, 3, 4, 2, 0.5)
    print('g17_trace_rnnmlp_rmsprop_decay: loss %.6f -> %.6f, lr' % (loss[0], loss[-1]), sorted(set(lrs.tolist()), reverse=True))
    save('g17_trace_rnnmlp_rmsprop_decay', S=S80, x=x, y=y, params0=p0, params_final=sd_np(m), loss=loss, metric=metric, lr=lrs,
         lr0=np.array(1e-2), alpha=np.array(0.9), period=np.array(2), rate=np.array(0.5), epochs=np.array(3), batch=np.array(4))


if __name__ == '__main__':
    assert mg.TOL > 0
    g17_plain()
    g17_adam_decay()
    g17_rnnmlp()
