"""Training harness of the epicenter-estimation driver on MI355X (counterpart of the reference's Modules/train_rnn_quake.py:18-480,
SURVEY.md rows 13 and H1): classification of the last state into regions. Same shape as Modules/train_rnn.py -- batch partition,
per-epoch permutation, loss -> backward -> optimiser step, validation every `validationInterval` steps, <name>Archit<label>.ckpt
checkpoints, learning-rate decay at the top of every epoch, batch-sharded data parallelism with one flat all-reduce per step -- with the
reference's classification behaviour:

  * labels are integers: nTrain or nTrain x 1 in any dtype, cast to int64 per batch (:220) and passed to the loss squeezed (:268);
  * names with 'GCRNN': archit(x [B][T][1][N], h0 = 0) (:252-256); other names with 'RNN': archit(x [B][T][1][N], h0, c0 = h0) with
    h0 = zeros(B, rnnStateFeat) (:257-262); other names ('Sel'): archit(x [B][T][N]) -- the window's T samples are the node features
    (:243, :265), NOT the (B*T) x 1 x N view of the regression harness;
  * the validation score is an accuracy: the best checkpoint is the first validation, then every strictly HIGHER one (:406-420).

The loss and both accuracies stay on the device: with Utils.miscTools.crossEntropyLoss the step's training accuracy is the hit count the
loss kernel produced in the same launch, read together with the loss in ONE device-to-host transfer per step.
"""
import time
import warnings

import numpy as np
import torch

from .. import ops
from ..optim import StepDecay
from ..parallel import FlatGradAllReduce, shard_range
from .train_rnn import (GraphedTrainStep, TrainableModel, batch_partition, train_step,  # noqa: F401  (re-exported: the drivers' surface)
                        _first_parameter, _is_gcrnn, _is_rnn, _rnn_forward)


def _gnn_forward(archit, x):
    """The reference's non-recurrent branch (train_rnn_quake.py:243, :265): x B x T x 1 x N -> archit(B x T x N), T = node features."""
    return archit(x.squeeze(2))


def _forward_of(key, m, rnnStateFeat):
    """yHat = fwd(archit, x [B][T][1][N]) for train_step; None = the GCRNN form archit(x, h0 = 0)."""
    if _is_gcrnn(key):
        return None
    if _is_rnn(key):
        return _rnn_forward(rnnStateFeat if rnnStateFeat is not None else m.archit.F_h)
    return _gnn_forward


def _logits(key, m, fwd, x, stateFeat):
    if fwd is not None:
        return fwd(m.archit, x)
    return m.archit(x, torch.zeros(x.shape[0], stateFeat, x.shape[3], dtype=x.dtype, device=x.device))


def _labels(y, n):
    """int64 labels [n] from n or n x 1 in any dtype (reference :220, :268)."""
    return torch.as_tensor(y).reshape(n).to(torch.int64)


def MultipleModels(modelsDict, xTrain, yTrain, xValid, yValid, nEpochs, batchSize, seqLen, stateFeat,
                   evaluate, validationInterval=5, rank=0, world=1, doPrint=False, rng=None, dataType=None, rnnStateFeat=None,
                   learningRateDecayRate=None, learningRateDecayPeriod=None):
    """Train every model of `modelsDict` (name -> TrainableModel) on the same batches; the model's call form follows its name (module
    docstring). xTrain: nTrain x (seqLen * N) or nTrain x seqLen x N (QuakeData's 'signals'), yTrain: nTrain or nTrain x 1 integer labels in
    any dtype (QuakeData's 'labels'); host or device tensors. evaluate(yHat, y) is the dataset's accuracy (QuakeData.evaluate /
    miscTools.accuracy), higher = better. It scores the validation set; the per-step training accuracy is the loss's own hit count when the
    loss provides one (`last_hits`, miscTools.crossEntropyLoss), else evaluate(yHat, y) -- either way one device-to-host transfer per step
    carries the loss and the accuracy together. With world > 1 each rank takes its shard of every batch (loss and training accuracy are the
    shard's) and the gradients are averaged by one flat all-reduce. rng, dataType, rnnStateFeat, learningRateDecayRate / Period: as
    train_rnn.MultipleModels. Returns dicts of per-step loss / accuracy / seconds per model, the validation accuracies, and bestScore /
    bestStep (the highest validation accuracy and the step it was measured at)."""
    if rng is None:
        rng = np.random.RandomState(20231) if world > 1 else np.random
    nTrain = xTrain.shape[0]
    sizes, index = batch_partition(nTrain, batchSize)
    fwds = {k: _forward_of(k, m, rnnStateFeat) for k, m in modelsDict.items()}
    p0 = _first_parameter(next(iter(modelsDict.values())).archit)
    dev = p0.device
    dt = dataType if dataType is not None else p0.dtype
    syncs = {k: ((m.optim.sync if hasattr(m.optim, 'sync') else FlatGradAllReduce(m.archit.parameters())) if world > 1 else None)
             for k, m in modelsDict.items()}
    yTrain = _labels(yTrain, nTrain)
    lossTrain = {k: [] for k in modelsDict}
    evalTrain = {k: [] for k in modelsDict}
    evalValid = {k: [] for k in modelsDict}
    timeTrain = {k: [] for k in modelsDict}
    best, bestStep = {}, {}
    schedulers = {}
    if learningRateDecayRate is not None and learningRateDecayPeriod is not None:
        schedulers = {k: StepDecay(m.optim, learningRateDecayPeriod, learningRateDecayRate) for k, m in modelsDict.items()}
    if xValid is not None:
        yv = _labels(yValid, xValid.shape[0]).to(dev)
    for epoch in range(nEpochs):
        perm = [int(i) for i in rng.permutation(nTrain)]
        if schedulers:
            with warnings.catch_warnings():
                # (torch's StepLR warns when it is stepped before the first optimiser step: that order is the reference's, kept on purpose)
                warnings.filterwarnings('ignore', message='Detected call of `lr_scheduler.step\\(\\)` before `optimizer.step\\(\\)`')
                for sched in schedulers.values():
                    sched.step()
            if doPrint and rank == 0:
                print('Epoch %d, learning rate = %.8f' % (epoch + 1, sched.get_last_lr()[0]))       # reference train_rnn_quake.py:208-209
        for b in range(len(sizes)):
            idx = perm[index[b]:index[b + 1]]
            nGlobal = len(idx)
            lo, hi = shard_range(nGlobal, rank, world)
            idx = idx[lo:hi]
            nLocal = len(idx)
            share = nLocal / float(nGlobal)                                       # this rank's weight in the flat all-reduce
            # (explicit shapes: an EMPTY shard -- a global batch smaller than the world -- cannot infer a -1)
            xb = xTrain[idx].reshape(nLocal, seqLen, xTrain[0].numel() // seqLen).to(dev, dt)
            yb = yTrain[idx].to(dev)
            for key, m in modelsDict.items():
                xo = (xb[:, :, m.order] if m.order is not None else xb).unsqueeze(2)      # B x T x 1 x N
                torch.cuda.synchronize() if dev.type == 'cuda' else None
                t0 = time.perf_counter()
                loss, yHat = train_step(m.archit, m.loss, m.optim, xo, yb, stateFeat, syncs[key], share if world > 1 else None, fwds[key])
                torch.cuda.synchronize() if dev.type == 'cuda' else None
                timeTrain[key].append(time.perf_counter() - t0)
                if yHat is None:                                                  # empty shard
                    lossTrain[key].append(float(loss))
                    evalTrain[key].append(float('nan'))
                    continue
                hits = getattr(m.loss, 'last_hits', None)
                acc = hits.to(torch.float64) / nLocal if hits is not None else torch.as_tensor(evaluate(yHat, yb)).to(loss.device, torch.float64)
                both = torch.stack([loss.to(torch.float64).reshape(()), acc.reshape(())]).tolist()      # ONE transfer: loss and accuracy
                lossTrain[key].append(both[0])
                evalTrain[key].append(both[1])
            step = epoch * len(sizes) + b
            if validationInterval and step % validationInterval == 0 and xValid is not None:
                nValid = xValid.shape[0]
                xv0 = xValid.reshape(nValid, seqLen, -1).to(dev, dt)
                for key, m in modelsDict.items():
                    xv = (xv0[:, :, m.order] if m.order is not None else xv0).unsqueeze(2)      # reference train_rnn_quake.py:347-353
                    with torch.no_grad():
                        score = float(evaluate(_logits(key, m, fwds[key], xv, stateFeat), yv))
                    evalValid[key].append(score)
                    if key not in best or score > best[key]:                     # first validation, then strictly higher (:406-420)
                        best[key], bestStep[key] = score, step
                        if rank == 0:
                            m.save(label='Best')
                    if doPrint and rank == 0:
                        print('[E %d B %d] %s valid accuracy %.4f' % (epoch + 1, b + 1, key, score))
        if rank == 0:
            for m in modelsDict.values():
                m.save(label='Last')
    return dict(lossTrain=lossTrain, evalTrain=evalTrain, evalValid=evalValid, timeTrain=timeTrain, bestScore=best, bestStep=bestStep)


def evaluate_checkpoints(modelsDict, xTest, yTest, seqLen, stateFeat, evaluate, rnnStateFeat=None, dataType=None, labels=('Best', 'Last')):
    """The driver's test phase (epicenterEstimation.py:1149-1245): load the `Best` and the `Last` checkpoint of every model and
    measure its accuracy on the test set under no_grad, the model called in the form its name asks for. Returns
    {label: {name: accuracy}}; the models are left with the last label's parameters loaded."""
    p0 = _first_parameter(next(iter(modelsDict.values())).archit)
    dev = p0.device
    dt = dataType if dataType is not None else p0.dtype
    nTest = xTest.shape[0]
    x0 = xTest.reshape(nTest, seqLen, -1).to(dev, dt)
    y = _labels(yTest, nTest).to(dev)
    out = {label: {} for label in labels}
    for label in labels:
        for key, m in modelsDict.items():
            m.load(label=label)
            ops.parameters_changed()
            x = (x0[:, :, m.order] if m.order is not None else x0).unsqueeze(2)
            with torch.no_grad():
                out[label][key] = float(evaluate(_logits(key, m, _forward_of(key, m, rnnStateFeat), x, stateFeat), y))
    return out
