#!/usr/bin/env python3
"""K-step prediction with gated GCRNNs on MI355X -- counterpart of the reference driver kStepPredGRNNs.py
(graph -> S = W/lambda_max -> data -> models -> train -> test; its lines 598-1677), reduced to the GCRNN models.

    python examples/kstep_prediction.py [--nodes 80] [--taps 5] [--seq 5] [--epochs 1] [--dtype f64]
    python examples/kstep_prediction.py --nodes 1000 --features 64 --seq 32 --dtype bf16 --ntrain 1024 --batch 256 --sparse

Defaults follow the reference driver (N=80 SBM 0.8/0.2, 5 taps, K=seqLen=5, F=20, batch 100, Adam 1e-3); --trainer ADAM|SGD|RMSprop,
--lr, --beta1, --beta2, --lr-decay-rate and --lr-decay-period are the driver's training options (kStepPredGRNNs.py:158-172). --dtype bf16 feeds
bf16 batches to fp32 master weights: all four variants (un-gated, time-, node- and edge-gated) then train on the fused kernels
(N <= 1024, F in {32, 64}; other shapes: composed path in fp32). --sparse draws the BASELINE configs[1] graph (mean degree ~10).
--models also accepts the driver's GNN models: 'Sel' (SelectionGNN([1, 8, 1], [10, 10], ReLU, NoPool), every time step a sample,
kStepPredGRNNs.py:197) and 'GCRNNGNN' / 'TimeGCRNNGNN' (a Selection-GNN head [F, 1], K = taps, final ReLU; the driver's [5, 1]
with F = 20 fails the reference's own shape assert), and 'RNNMLP' (the driver's RNN baseline: RNNforRegression(1, --rnn-features,
'tanh', [1], ReLU), kStepPredGRNNs.py:285-301).
"""
import argparse
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import gated_gcrnns_amd.Modules.architectures as archit
import gated_gcrnns_amd.Utils.graphML as gml
from gated_gcrnns_amd.Modules.train_rnn import MultipleModels, TrainableModel
from gated_gcrnns_amd.Utils import dataTools, miscTools
from gated_gcrnns_amd.optim import TRAINERS, make_trainer


MODELS = ('GCRNNMLP', 'TimeGCRNNMLP', 'NodeGCRNNMLP', 'EdgeGCRNNMLP', 'Sel', 'GCRNNGNN', 'TimeGCRNNGNN', 'RNNMLP')


def main(argv=None):
    """Returns {model name: dict(loss=[per-step training loss], score=test metric, ms=median ms per batch)}."""
    ap = argparse.ArgumentParser()
    ap.add_argument('--nodes', type=int, default=80)
    ap.add_argument('--taps', type=int, default=5)
    ap.add_argument('--seq', type=int, default=5)
    ap.add_argument('--features', type=int, default=20)
    ap.add_argument('--epochs', type=int, default=1)
    ap.add_argument('--batch', type=int, default=100)
    ap.add_argument('--ntrain', type=int, default=2000)
    ap.add_argument('--dtype', default='f64', choices=['f32', 'f64', 'bf16'])
    ap.add_argument('--sparse', action='store_true', help='SBM with p_in 0.04 / p_out 0.0025 (BASELINE configs[1]) instead of 0.8 / 0.2')
    ap.add_argument('--models', default='GCRNNMLP,TimeGCRNNMLP,NodeGCRNNMLP,EdgeGCRNNMLP',
                    help='comma-separated, of ' + ','.join(MODELS))
    ap.add_argument('--rnn-features', type=int, default=1, help="RNNMLP's state features (the driver's rnnStateFeat)")
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--optim', default='flat', choices=['flat', 'torch'], help='flat: optim.FlatAdam / FlatSGD / FlatRMSprop (one kernel over '
                    'the flat parameter / gradient buffers); torch: the torch.optim class as in the reference driver')
    ap.add_argument('--trainer', default='ADAM', choices=TRAINERS, help="the driver's `trainer` (kStepPredGRNNs.py:158)")
    ap.add_argument('--lr', type=float, default=1e-3, help="the driver's learningRate")
    ap.add_argument('--beta1', type=float, default=0.9, help="Adam's beta1; RMSprop's alpha, as in the driver")
    ap.add_argument('--beta2', type=float, default=0.999)
    ap.add_argument('--lr-decay-rate', type=float, default=None, help="the driver's learningRateDecayRate (give both decay options to turn decay on)")
    ap.add_argument('--lr-decay-period', type=int, default=None, help="the driver's learningRateDecayPeriod, in epochs; the schedule is stepped "
                    'at the top of every epoch as in the reference')
    args = ap.parse_args(argv)
    unknown = [n for n in args.models.split(',') if n not in MODELS]
    if unknown:
        ap.error('unknown model(s) %s; choose from %s' % (','.join(unknown), ','.join(MODELS)))
    dt = torch.float64 if args.dtype == 'f64' else torch.float32       # parameter dtype (bf16: fp32 master weights)
    data_dt = torch.bfloat16 if args.dtype == 'bf16' else dt
    torch.set_default_dtype(dt)                                   # the reference driver runs in float64 (line 44)
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(args.seed)
    torch.manual_seed(args.seed)
    W = dataTools.sbm_adjacency(args.nodes, 5, 0.04, 0.0025, rng) if args.sparse else dataTools.sbm_adjacency(args.nodes, 5, 0.8, 0.2, rng)
    S = dataTools.normalised_gso(W)
    K = args.seq
    data = dataTools.KStepPrediction(W, K, args.ntrain, 200, 200, horizon=2 * K, rng=rng, dataType=dt)
    saveDir = tempfile.mkdtemp(prefix='kstep_')
    models = {}
    for name, tg, sg in (('GCRNNMLP', False, None), ('TimeGCRNNMLP', True, None), ('NodeGCRNNMLP', False, 'node'),
                         ('EdgeGCRNNMLP', False, 'edge')):
        if name not in args.models.split(','):
            continue
        m = archit.GatedGCRNNforRegression(1, args.features, args.taps, args.taps, torch.tanh, torch.nn.ReLU, [1], S, True,
                                           time_gating=tg, spatial_gating=sg, mlpType='multipMlp').to(dev)
        opt = make_trainer(args.trainer, m.parameters(), args.lr, args.beta1, args.beta2, flat=args.optim == 'flat')      # kStepPredGRNNs.py:706-715
        models[name] = TrainableModel(m, miscTools.batchTimeL1Loss, opt, name, saveDir)
    for name in args.models.split(','):
        if name == 'Sel':
            m = archit.SelectionGNN([1, 8, 1], [10, 10], True, torch.nn.ReLU, [args.nodes] * 2, gml.NoPool, [1, 1], [], S)
        elif name in ('GCRNNGNN', 'TimeGCRNNGNN'):
            m = archit.GatedGCRNNforRegression(1, args.features, args.taps, args.taps, torch.tanh, torch.nn.ReLU, [], S, True,
                                               name == 'TimeGCRNNGNN', None, 'oneMlp', torch.nn.ReLU, [args.features, 1], [args.taps],
                                               [args.nodes], gml.NoPool, [1])
        elif name == 'RNNMLP':
            m = archit.RNNforRegression(1, args.rnn_features, 'tanh', [1], torch.nn.ReLU, S, True)
        else:
            continue
        m = m.to(dev)
        opt = make_trainer(args.trainer, m.parameters(), args.lr, args.beta1, args.beta2, flat=args.optim == 'flat')
        models[name] = TrainableModel(m, miscTools.batchTimeL1Loss, opt, name, saveDir)
    xT, yT = data.getSamples('train')
    xV, yV = data.getSamples('valid')
    out = MultipleModels(models, xT, yT, xV, yV, args.epochs, args.batch, data.seqLen, args.features,
                         data.evaluate, validationInterval=5, rng=rng, doPrint=False, dataType=data_dt, rnnStateFeat=args.rnn_features,
                         learningRateDecayRate=args.lr_decay_rate, learningRateDecayPeriod=args.lr_decay_period)
    xE, yE = data.getSamples('test')
    xE = xE.view(xE.shape[0], data.seqLen, -1).to(dev, data_dt).unsqueeze(2)
    yE = yE.view(yE.shape[0], data.seqLen, -1).to(dev, data_dt).unsqueeze(2)
    result = {}
    for name, tm in models.items():
        tm.load('Best')
        with torch.no_grad():
            if name == 'Sel':                                             # every time step a sample (reference train_rnn.py:243)
                yS = tm.archit(xE.reshape(-1, 1, args.nodes).to(dt)).unsqueeze(1)
                score = float(data.evaluate(yS.to(yE.dtype), yE.reshape(-1, 1, args.nodes)))
            elif name == 'RNNMLP':                                        # reference train_rnn.py:246-251
                h0 = torch.zeros(xE.shape[0], args.rnn_features, device=dev, dtype=data_dt)
                score = float(data.evaluate(tm.archit(xE, h0, h0).to(yE.dtype), yE))
            else:
                h0 = torch.zeros(xE.shape[0], args.features, args.nodes, device=dev, dtype=data_dt)
                score = float(data.evaluate(tm.archit(xE, h0).to(yE.dtype), yE))
        t = np.median(out['timeTrain'][name])
        print('%-14s test RMSE-metric %.4f   loss %.4f -> %.4f   median %.1f ms/batch (%.0f seq/s)' % (
            name, score, out['lossTrain'][name][0], out['lossTrain'][name][-1], 1e3 * t, args.batch / t))
        result[name] = dict(loss=list(out['lossTrain'][name]), score=score, ms=1e3 * t)
    return result


if __name__ == '__main__':
    main()
