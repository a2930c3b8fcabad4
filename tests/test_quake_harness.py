"""GPU: the epicenter-estimation driver's harness (Modules/train_rnn_quake.py) with the HIP cross-entropy loss: the reference's training
traces (golden G18: its models under torch.optim.Adam + nn.CrossEntropyLoss on the CPU in float64, tests/golden/make_golden_quake.py), the
harness's own behaviour (call forms, best = highest, checkpoints, test phase), captured training steps with int64 labels, and the example.

Bounds of the fp64 traces: per-step loss 1e-9 and final parameters 1e-8 (G6 / G16 / G17's, tests/test_training_trace.py), the training,
validation and test hit counts EXACTLY: the fixture's generator asserts that the two largest reference logits of every row it scores are at
least 1e-4 apart, so parameters 1e-8 away cannot change an argmax. No row is exempted."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
T, F1, K1, RNN_F, REGIONS = 20, 20, 4, 21, 11
NAMES = ['GCRNNMLP', 'TimeGCRNNMLP', 'GCRNNGNN', 'RNNMLP', 'Sel']


def _build(name, S):
    import gated_gcrnns_amd.Modules.architectures as archit
    import gated_gcrnns_amd.Utils.graphML as gml
    N = S.shape[0]
    if name == 'Sel':
        return archit.SelectionGNN([T, 21], [K1], True, torch.nn.ReLU, [N], gml.NoPool, [1], [REGIONS], S)
    if name == 'RNNMLP':
        return archit.RNNforClassification(1, RNN_F, 'tanh', [REGIONS], torch.nn.ReLU, S, True)
    head = dict(finalNonlinearity=torch.nn.ReLU, dimNodeSignals=[F1, 1], nFilterTaps=[K1], nSelectedNodes=[N],
                poolingFunction=gml.NoPool, poolingSize=[1]) if name.endswith('GNN') else {}
    return archit.GatedGCRNNforClassification(1, F1, K1, K1, torch.tanh, torch.nn.ReLU, [REGIONS], S, True,
                                              time_gating=name.startswith('Time'), spatial_gating=None, **head)


def _model(name, g, S):
    m = _build(name, S).double()
    m.load_state_dict({k: torch.tensor(v) for k, v in g['params0'].items()})
    return m.to(DEV)


class _Replay(object):
    """rng of MultipleModels that replays the fixture's epoch permutations."""

    def __init__(self, perms):
        self.perms = [list(p) for p in perms]

    def permutation(self, n):
        p = self.perms.pop(0)
        assert len(p) == n
        return np.array(p)


def _counts(values, sizes):
    return [int(round(v * n)) for v, n in zip(values, sizes)]


@pytest.mark.parametrize('name,flat', [(n, False) for n in NAMES] + [('GCRNNMLP', True), ('Sel', True)])
def test_g18_twenty_steps_match_reference(name, flat, tmp_path):
    from gated_gcrnns_amd import optim
    from gated_gcrnns_amd.Modules.train_rnn_quake import MultipleModels, TrainableModel, evaluate_checkpoints
    from gated_gcrnns_amd.Utils.miscTools import CrossEntropyLoss, accuracy
    d = load_golden('g18_quake_data')
    g = load_golden('g18_trace_' + name)
    assert str(g['loop']) == 'restated' and float(g['min_gap']) >= 1e-4
    m = _model(name, g, d['S'][0])
    opt = optim.make_trainer('ADAM', m.parameters(), float(g['lr']), 0.9, 0.999, flat=flat)
    models = {name: TrainableModel(m, CrossEntropyLoss(), opt, name, str(tmp_path))}
    kw = dict(seqLen=T, stateFeat=F1, evaluate=accuracy, rnnStateFeat=RNN_F)
    out = MultipleModels(models, torch.tensor(d['train_signals']), torch.tensor(d['train_labels']), torch.tensor(d['valid_signals']),
                         torch.tensor(d['valid_labels']), nEpochs=int(g['epochs']), batchSize=int(g['batch']),
                         validationInterval=int(g['valid_every']), rng=_Replay(g['perms']), **kw)
    sizes = [5, 5, 5, 3] * int(g['epochs'])
    el = np.max(np.abs(np.array(out['lossTrain'][name]) - g['loss']))
    sd = m.state_dict()
    ep = max(np.max(np.abs(sd[k].cpu().numpy() - v)) for k, v in g['params20'].items())
    hits = _counts(out['evalTrain'][name], sizes)
    nV = d['valid_labels'].shape[0]
    valid = _counts(out['evalValid'][name], [nV] * 4)
    test = evaluate_checkpoints(models, torch.tensor(d['test_signals']), torch.tensor(d['test_labels']), **kw)
    nT = d['test_labels'].shape[0]
    print('G18 %s flat=%s: max|loss - ref| = %.3g, max|param - ref| = %.3g, hits %s ref %s, valid %s ref %s, test Last %.3f ref %.3f'
          % (name, flat, el, ep, hits, g['hits'].tolist(), valid, _counts(g['valid_accuracy'], [nV] * 4), test['Last'][name],
             float(g['test_accuracy'])))
    assert len(out['lossTrain'][name]) == 20
    assert el <= 1e-9
    assert ep <= 1e-8
    assert hits == g['hits'].tolist()                                   # exactly
    assert np.max(np.abs(np.array(out['evalTrain'][name]) - g['accuracy'])) <= 1e-15      # (hits / B against the reference's 1 - errors / B)
    assert valid == _counts(g['valid_accuracy'], [nV] * 4)
    assert int(round(test['Last'][name] * nT)) == int(round(float(g['test_accuracy']) * nT))
    assert set(test) == {'Best', 'Last'} and 0.0 <= test['Best'][name] <= 1.0


class _SelSpy(torch.nn.Module):
    """A Selection GNN that insists on the epicenter harness's input form: B x T x N, the window's samples as node features."""

    def __init__(self, sel):
        super().__init__()
        self.sel = sel
        self.shapes = []

    def forward(self, x):
        assert x.dim() == 3 and x.shape[1] == T and x.shape[2] == 59, tuple(x.shape)
        self.shapes.append(tuple(x.shape))
        return self.sel(x)


def test_harness_steps_input_forms_best_is_highest_and_checkpoints(tmp_path):
    from gated_gcrnns_amd.Modules import train_rnn, train_rnn_quake
    from gated_gcrnns_amd.Utils.miscTools import CrossEntropyLoss, accuracy
    d = load_golden('g18_quake_data')
    S = d['S'][0]
    torch.manual_seed(3)
    spy = _SelSpy(_build('Sel', S).double()).to(DEV)
    gc = _build('GCRNNMLP', S).double().to(DEV)
    saves, snaps, step = [], [], [0]

    class Recording(train_rnn_quake.TrainableModel):
        def save(self, label=''):
            saves.append((self.name, label, step[0]))
            super().save(label)

    models = {'Sel': Recording(spy, CrossEntropyLoss(), torch.optim.Adam(spy.parameters(), lr=1e-2), 'Sel', str(tmp_path)),
              'GCRNNMLP': Recording(gc, CrossEntropyLoss(), torch.optim.Adam(gc.parameters(), lr=1e-2), 'GCRNNMLP', str(tmp_path))}
    script = {'Sel': [0.3, 0.5, 0.4, 0.4, 0.5, 0.1], 'GCRNNMLP': [0.2, 0.2, 0.1, 0.6, 0.6, 0.0]}
    calls = []

    def evaluate(yHat, y):                                     # validation only: the training accuracy is the loss kernel's hit count
        assert tuple(yHat.shape) == (6, REGIONS) and y.dtype == torch.int64 and tuple(y.shape) == (6,)
        key = 'Sel' if len(calls) % 2 == 0 else 'GCRNNMLP'
        calls.append(key)
        step[0] = (len(calls) - 1) // 2
        snaps.append((key, {k: v.detach().clone() for k, v in models[key].archit.state_dict().items()}))
        return script[key][(len(calls) - 1) // 2]

    x, y = torch.tensor(d['train_signals'][:13]), torch.tensor(d['train_labels'][:13])      # 13 windows: batches of 5, 5, 3
    out = train_rnn_quake.MultipleModels(models, x, y, torch.tensor(d['valid_signals']), torch.tensor(d['valid_labels']), nEpochs=2,
                                         batchSize=5, seqLen=T, stateFeat=F1, evaluate=evaluate, validationInterval=1,
                                         rng=np.random.RandomState(0))
    assert all(len(out[k][n]) == 6 for k in ('lossTrain', 'evalTrain', 'evalValid', 'timeTrain') for n in models)
    assert spy.shapes == [(5, T, 59), (6, T, 59), (5, T, 59), (6, T, 59), (3, T, 59), (6, T, 59)] * 2
    assert all(0.0 <= a <= 1.0 for n in models for a in out['evalTrain'][n])
    assert out['bestScore'] == {'Sel': 0.5, 'GCRNNMLP': 0.6} and out['bestStep'] == {'Sel': 1, 'GCRNNMLP': 3}   # strictly higher only
    assert [s for s in saves if s[0] == 'Sel'] == [('Sel', 'Best', 0), ('Sel', 'Best', 1), ('Sel', 'Last', 2), ('Sel', 'Last', 5)]
    assert [s for s in saves if s[0] == 'GCRNNMLP'] == [('GCRNNMLP', 'Best', 0), ('GCRNNMLP', 'Last', 2), ('GCRNNMLP', 'Best', 3),
                                                       ('GCRNNMLP', 'Last', 5)]
    ck = os.path.join(str(tmp_path), 'savedModels')
    best = torch.load(os.path.join(ck, 'SelArchitBest.ckpt'))
    want = [s for k, s in snaps if k == 'Sel'][1]                                     # the parameters of step 2's validation
    assert all(torch.equal(best[k].to(DEV), want[k]) for k in want)
    last = torch.load(os.path.join(ck, 'SelArchitLast.ckpt'))
    assert all(torch.equal(last[k].to(DEV), v) for k, v in spy.state_dict().items())
    acc = train_rnn_quake.evaluate_checkpoints(models, torch.tensor(d['test_signals']), torch.tensor(d['test_labels']), seqLen=T,
                                               stateFeat=F1, evaluate=accuracy)
    assert set(acc) == {'Best', 'Last'} and all(set(acc[k]) == set(models) and all(0.0 <= v <= 1.0 for v in acc[k].values()) for k in acc)
    # the regression harness would hand the same model (B*T) x 1 x N: its shape assert fails there
    with pytest.raises(AssertionError):
        train_rnn.MultipleModels({'Sel': models['Sel']}, x.reshape(13, T, 59), x.reshape(13, T, 59), None, None, 1, 5, T, F1,
                                 evaluate=lambda a, b: 0.0, validationInterval=0)


@pytest.mark.parametrize('two_graphs', [False, True])
def test_graphed_train_step_with_int64_labels_replays_eager_bits(two_graphs):
    from gated_gcrnns_amd import optim
    from gated_gcrnns_amd.Modules.train_rnn_quake import GraphedTrainStep, train_step
    from gated_gcrnns_amd.Utils.miscTools import CrossEntropyLoss
    d = load_golden('g18_quake_data')
    g = load_golden('g18_trace_GCRNNMLP')
    S = d['S'][0]
    x = torch.tensor(d['train_signals'], device=DEV).reshape(-1, T, 1, 59)
    y = torch.tensor(d['train_labels'], device=DEV).reshape(-1).to(torch.int64)
    me, mg = _model('GCRNNMLP', g, S), _model('GCRNNMLP', g, S)
    oe = optim.make_trainer('ADAM', me.parameters(), 1e-3, 0.9, 0.999, flat=True)
    og = optim.make_trainer('ADAM', mg.parameters(), 1e-3, 0.9, 0.999, flat=True)
    le, lg = CrossEntropyLoss(), CrossEntropyLoss()
    stepper = GraphedTrainStep(mg, lg, og, x[:6], y[:6], F1, sync=og.sync if two_graphs else None)      # 3 eager warm-up steps inside
    assert stepper.captured and (stepper.graph_step is not None) == two_graphs and stepper.y.dtype == torch.int64
    for _ in range(3):
        train_step(me, le, oe, x[:6], y[:6], F1)
    for it in range(5):
        xb, yb = x[it:it + 6], y[it:it + 6]                                        # fresh inputs every replay
        loss_e, yhat_e = train_step(me, le, oe, xb, yb, F1)
        loss_g, yhat_g = stepper(xb, yb)
        assert torch.equal(loss_e, loss_g) and torch.equal(yhat_e, yhat_g), it
        assert torch.equal(le.last_hits, lg.last_hits) and int(lg.last_hits) == int((yhat_g.argmax(dim=1) == yb).sum())
        assert all(torch.equal(a, b) for a, b in zip(me.parameters(), mg.parameters())), it


def test_example_through_the_harness_with_the_hip_loss(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import epicenter_estimation
    old = torch.get_default_dtype()                          # (main() sets the drivers' float64 default: put the process's back)
    try:
        out = epicenter_estimation.main(['--harness', '--loss', 'hip', '--seq', '20', '--epochs', '4', '--valid-interval', '20',
                                         '--save-dir', str(tmp_path)])
        print('example --harness --loss hip: loss %.3f -> %.3f, test accuracy Best %.3f Last %.3f, %.2f ms/step'
              % (out['loss'][0], out['loss'][-1], out['best_accuracy'], out['last_accuracy'], out['ms_per_step']))
        assert len(out['loss']) == 4 * 20
        assert np.mean(out['loss'][-10:]) < np.mean(out['loss'][:10])
        assert 0.0 <= out['accuracy'] <= 1.0 and 0.0 <= out['best_accuracy'] <= 1.0 and out['accuracy'] == out['last_accuracy']
        assert out['ms_per_step'] > 0
        # the plain loop with the HIP loss: same keys as before
        out = epicenter_estimation.main(['--loss', 'hip', '--seq', '20', '--steps', '60'])
        assert np.mean(out['loss'][-10:]) < np.mean(out['loss'][:10]) and 0.0 <= out['accuracy'] <= 1.0
    finally:
        torch.set_default_dtype(old)
