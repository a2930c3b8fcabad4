#!/usr/bin/env python3
"""Epicenter-region classification with a gated GCRNN on MI355X -- counterpart of the reference driver
epicenterEstimation.py (its lines 445-1245: seismograph graph -> S = A / |lambda_max| -> GatedGCRNNforClassification on the
last state -> cross-entropy -> accuracy), BASELINE configs[3].

The reference's recordings (X.p, y.p; dataTools.py:1466-1467) are not part of its repository, so the waves here are
SYNTHETIC: a pulse is released at a random station and spreads over the 59-station graph of the reference
(tests/golden/adj59.npy) with attenuation and sensor noise; the label is the region (one of 11 contiguous groups of
stations) of the source. Same tensor shapes and model as the driver: x is B x T x 1 x 59, 11 classes.

    python examples/epicenter_estimation.py [--seq 200] [--taps 3] [--steps 600] [--lr 5e-3] [--time-gating] [--dtype f64]
    python examples/epicenter_estimation.py --models Sel,GCRNNGNN,TimeGCRNNGNN
    python examples/epicenter_estimation.py --trainer RMSprop --lr 1e-3 --lr-decay-rate 0.9 --lr-decay-period 1 --steps-per-epoch 100
    python examples/epicenter_estimation.py --loss hip --harness --epochs 6 --valid-interval 10

--loss hip takes the loss, its gradient and the accuracy from the one-pass HIP cross-entropy kernel (Utils/miscTools.crossEntropyLoss /
accuracy) instead of torch.nn.CrossEntropyLoss and an argmax on the host. --harness trains through the driver's own harness,
Modules/train_rnn_quake.MultipleModels (epochs over the training windows in batches of --batch, validation every --valid-interval steps on
one half of the held-out windows, Best / Last checkpoints), then runs its test phase (evaluate_checkpoints) on the other half.

--models picks the driver's other models (epicenterEstimation.py:150-153, 180-196, 258-280): 'Sel' = SelectionGNN([T, 21], [taps],
ReLU, NoPool, MLP [11]) on the window's T samples as node features, 'GCRNNGNN' / 'TimeGCRNNGNN' = the gated GCRNN with a
Selection-GNN head [F, 1], K = taps, MLP [11], final ReLU, 'RNNMLP' = the driver's RNN baseline RNNforClassification(1,
--rnn-features, 'tanh', [11], ReLU) on the flattened window (epicenterEstimation.py:151, 172, 284-300). Default: the MLP-head GCRNN ('TimeGCRNNMLP' with --time-gating).

Measured on one MI355X (fp64, batch 100): T=200 3.6 ms per optimiser step, 84 % test accuracy after 600 steps (chance 9 %);
T=50 1.1 ms per step, 99.8 %. The time-gated variant trains at 2.0 ms per step (T=50) but needs the reference's
lr = 1e-3 and thousands of steps on this task (its gates collapse at 5e-3; same curve on both gate implementations).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import gated_gcrnns_amd.Modules.architectures as archit
import gated_gcrnns_amd.Utils.graphML as gml
from gated_gcrnns_amd.Modules import train_rnn_quake
from gated_gcrnns_amd.Modules.train_rnn import train_step
from gated_gcrnns_amd.Utils import miscTools
from gated_gcrnns_amd.Utils import dataTools
from gated_gcrnns_amd.optim import TRAINERS, StepDecay, make_trainer


synthetic_waves = dataTools.synthetic_waves


def run_harness(args, name, model, loss, opt, xtr, ytr, xte, yte):
    """The driver's training and test phases (epicenterEstimation.py:1128-1245) on the synthetic windows."""
    import tempfile
    evaluate = miscTools.accuracy if args.loss == 'hip' else \
        (lambda yHat, y: (yHat.argmax(dim=1) == y.reshape(-1)).to(torch.float64).mean())
    half = xte.shape[0] // 2
    tm = train_rnn_quake.TrainableModel(model, loss, opt, name, args.save_dir or tempfile.mkdtemp(prefix='epicenter_'))
    kw = dict(stateFeat=args.features, evaluate=evaluate, rnnStateFeat=args.rnn_features)
    out = train_rnn_quake.MultipleModels({name: tm}, torch.tensor(xtr), torch.tensor(ytr), torch.tensor(xte[:half]), torch.tensor(yte[:half]),
                                         nEpochs=args.epochs, batchSize=args.batch, seqLen=args.seq, validationInterval=args.valid_interval,
                                         learningRateDecayRate=args.lr_decay_rate, learningRateDecayPeriod=args.lr_decay_period, **kw)
    test = train_rnn_quake.evaluate_checkpoints({name: tm}, torch.tensor(xte[half:]), torch.tensor(yte[half:]), seqLen=args.seq, **kw)
    losses = out['lossTrain'][name]
    ms = 1e3 * float(np.median(out['timeTrain'][name][3:]))
    print('%s classification through the harness, T=%d %s, %d steps: loss %.3f -> %.3f, best validation accuracy %.3f (step %d), test accuracy '
          'Best %.3f / Last %.3f (chance %.3f), median %.2f ms/step' % (name, args.seq, args.dtype, len(losses), losses[0], losses[-1],
                                                                         out['bestScore'][name], out['bestStep'][name], test['Best'][name],
                                                                         test['Last'][name], 1 / 11, ms))
    return {'loss': losses, 'accuracy': test['Last'][name], 'ms_per_step': ms, 'best_accuracy': test['Best'][name],
            'last_accuracy': test['Last'][name]}


MODELS = ('GCRNNMLP', 'TimeGCRNNMLP', 'Sel', 'GCRNNGNN', 'TimeGCRNNGNN', 'RNNMLP')


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--seq', type=int, default=200)
    ap.add_argument('--taps', type=int, default=3)
    ap.add_argument('--features', type=int, default=20)
    ap.add_argument('--batch', type=int, default=100)
    ap.add_argument('--steps', type=int, default=600)
    ap.add_argument('--lr', type=float, default=5e-3, help='the reference driver uses 1e-3 over many epochs')
    ap.add_argument('--trainer', default='ADAM', choices=TRAINERS, help="the driver's `trainer` (epicenterEstimation.py, same block as the k-step driver)")
    ap.add_argument('--beta1', type=float, default=0.9, help="Adam's beta1; RMSprop's alpha, as in the driver")
    ap.add_argument('--beta2', type=float, default=0.999)
    ap.add_argument('--optim', default='torch', choices=['flat', 'torch'], help='torch: the torch.optim class as in the reference driver; '
                    'flat: optim.FlatAdam / FlatSGD / FlatRMSprop (one kernel over the flat parameter / gradient buffers)')
    ap.add_argument('--lr-decay-rate', type=float, default=None, help="the driver's learningRateDecayRate (give both decay options to turn decay on)")
    ap.add_argument('--lr-decay-period', type=int, default=None, help="the driver's learningRateDecayPeriod, in epochs")
    ap.add_argument('--steps-per-epoch', type=int, default=None, help='this example draws --steps random batches without epochs: an "epoch" of the '
                    'decay schedule is this many steps (default: all steps = one epoch); the schedule is stepped at the top of each, as in the reference')
    ap.add_argument('--time-gating', action='store_true')
    ap.add_argument('--rnn-features', type=int, default=21, help="RNNMLP's state features (the driver's rnnStateFeat)")
    ap.add_argument('--dtype', default='f64', choices=['f32', 'f64'])
    ap.add_argument('--models', default=None, help='comma-separated, of ' + ','.join(MODELS) + ' (default: one MLP-head GCRNN)')
    ap.add_argument('--loss', default='torch', choices=['torch', 'hip'], help='torch: nn.CrossEntropyLoss and a host argmax; hip: the one-pass '
                    'cross-entropy kernel for loss, gradient and accuracy')
    ap.add_argument('--harness', action='store_true', help='train through Modules/train_rnn_quake.MultipleModels and test its Best / Last checkpoints')
    ap.add_argument('--epochs', type=int, default=3, help='--harness: epochs over the training windows (instead of --steps random batches)')
    ap.add_argument('--valid-interval', type=int, default=10, help="--harness: the driver's validationInterval, in steps")
    ap.add_argument('--save-dir', default=None, help='--harness: where the checkpoints go (default: a temporary directory)')
    args = ap.parse_args(argv)
    names = args.models.split(',') if args.models else ['TimeGCRNNMLP' if args.time_gating else 'GCRNNMLP']
    if any(n not in MODELS for n in names):
        ap.error('unknown model in %s; choose from %s' % (args.models, ','.join(MODELS)))
    dt = torch.float64 if args.dtype == 'f64' else torch.float32
    torch.set_default_dtype(dt)                                      # the reference driver runs in float64
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    adj = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'adj59.npy'))
    S = dataTools.normalised_gso(adj)                                # A / |lambda_max| (epicenterEstimation.py:619)
    N = S.shape[0]
    regions = (np.arange(N) * 11) // N                               # 11 contiguous groups of stations
    xtr, ytr = synthetic_waves(S, 20 * args.batch, args.seq, regions, rng)
    xte, yte = synthetic_waves(S, 5 * args.batch, args.seq, regions, rng)
    to_x = lambda a: torch.tensor(a, dtype=dt, device=dev).unsqueeze(2)              # B x T x 1 x N
    xtr_d, ytr_d = to_x(xtr), torch.tensor(ytr, device=dev)
    xe = to_x(xte)
    results = {}
    for name in names:
        torch.manual_seed(0)
        gnn = name == 'Sel'
        if gnn:
            model = archit.SelectionGNN([args.seq, 21], [args.taps], True, torch.nn.ReLU, [N], gml.NoPool, [1], [11], S).to(dev)
            fwd = lambda a, x: a(x.squeeze(2))                           # the T samples of a window are the node features
        elif name == 'RNNMLP':
            model = archit.RNNforClassification(1, args.rnn_features, 'tanh', [11], torch.nn.ReLU, S, True).to(dev)

            def fwd(a, x):
                h0 = torch.zeros(x.shape[0], args.rnn_features, dtype=x.dtype, device=x.device)
                return a(x, h0, h0)                                      # c0 = h0 (reference train_rnn.py:248-250)
        else:
            tg = name.startswith('Time')
            head = dict(finalNonlinearity=torch.nn.ReLU, dimNodeSignals=[args.features, 1], nFilterTaps=[args.taps], nSelectedNodes=[N],
                        poolingFunction=gml.NoPool, poolingSize=[1]) if name.endswith('GNN') else {}
            model = archit.GatedGCRNNforClassification(1, args.features, args.taps, args.taps, torch.tanh, torch.nn.ReLU, [11], S, True,
                                                       time_gating=tg, spatial_gating=None, **head).to(dev)
            fwd = None
        opt = make_trainer(args.trainer, model.parameters(), args.lr, args.beta1, args.beta2, flat=args.optim == 'flat')
        decay = StepDecay(opt, args.lr_decay_period, args.lr_decay_rate) if args.lr_decay_rate is not None and args.lr_decay_period is not None else None
        per_epoch = args.steps_per_epoch or max(args.steps, 1)
        ce = miscTools.CrossEntropyLoss() if args.loss == 'hip' else torch.nn.CrossEntropyLoss()
        if args.harness:
            results[name] = run_harness(args, name, model, ce, opt, xtr, ytr, xte, yte)
            continue
        times, first, losses = [], None, []
        for it in range(args.steps):
            if decay is not None and it % per_epoch == 0:
                decay.step()                                             # top of the epoch, before its first batch (reference train_rnn.py:197-200)
            idx = torch.tensor(rng.choice(xtr.shape[0], args.batch, replace=False), device=dev)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            loss, _ = train_step(model, ce, opt, xtr_d[idx], ytr_d[idx], args.features, forward=fwd)
            torch.cuda.synchronize(); times.append(time.perf_counter() - t0)
            first = float(loss) if first is None else first
            losses.append(float(loss))
        with torch.no_grad():
            if gnn:
                logits = model(xe.squeeze(2))
            elif name == 'RNNMLP':
                h0 = torch.zeros(xe.shape[0], args.rnn_features, dtype=dt, device=dev)
                logits = model(xe, h0, h0)
            else:
                logits = model(xe, torch.zeros(xe.shape[0], args.features, N, dtype=dt, device=dev))
            if args.loss == 'hip':
                acc = float(miscTools.accuracy(logits, torch.tensor(yte, device=dev)))
            else:
                acc = float((logits.argmax(dim=1).cpu() == torch.tensor(yte)).double().mean())
        ms = 1e3 * float(np.median(times[3:]))
        print('%s classification N=%d T=%d K=%d F=%d %s: loss %.3f -> %.3f, test accuracy %.3f (chance %.3f), '
              'median %.2f ms/step (%.0f seq/s)' % (name, N, args.seq, args.taps, args.features, args.dtype, first, float(loss), acc,
                                                   1 / 11, ms, args.batch / (ms / 1e3)))
        results[name] = {'loss': losses, 'accuracy': acc, 'ms_per_step': ms}
    return results[names[0]] if len(names) == 1 else results


if __name__ == '__main__':
    main()
