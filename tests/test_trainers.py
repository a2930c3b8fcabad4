"""GPU: the drivers' trainers and learning-rate decay on the flat-buffer HIP kernels (gcrnn_sgd_flat, gcrnn_rmsprop_flat,
gcrnn_adam_flat_dlr): the reference's traces (golden G17: torch.optim.SGD / RMSprop / Adam + StepLR on the CPU in float64), decay
under a captured training step, bit-identity of the two Adam paths, launch counts, argument checks, checkpoints and the examples.

The bounds on the fp64 traces are G6's (tests/test_training_trace.py: loss 1e-9, metric 1e-8, parameters 1e-8): the same forward and
backward kernels produce the gradients, and the optimiser steps are element-wise fp64 arithmetic in torch's order."""
import collections
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')


def _g6_model(g, dt=torch.float64):
    import gated_gcrnns_amd.Modules.architectures as archit
    m = archit.GatedGCRNNforRegression(1, 20, 3, 3, torch.tanh, torch.nn.ReLU, [1], g['S'][0], True,
                                       time_gating=False, spatial_gating=None, mlpType='multipMlp').double()
    m.load_state_dict({k: torch.tensor(v) for k, v in g['params0'].items()})
    return m.to(dt).to(DEV)


def _optimiser(kind, params, flat, lr=None):
    """The three trainers as optim.make_trainer / the reference build them; hyper-parameters of the G17 fixtures."""
    from gated_gcrnns_amd import optim
    if kind == 'sgd':
        return optim.make_trainer('SGD', params, 0.02 if lr is None else lr, 0.9, 0.999, flat=flat)
    if kind == 'rmsprop':
        return optim.make_trainer('RMSprop', params, 1e-3 if lr is None else lr, 0.9, 0.999, flat=flat)
    return optim.make_trainer('ADAM', params, 1e-3 if lr is None else lr, 0.9, 0.999, flat=flat)


def _lr_of(opt):
    return opt.param_groups[0]['lr'] if isinstance(opt, torch.optim.Optimizer) else opt.lr


@pytest.mark.parametrize('flat', [True, False])
@pytest.mark.parametrize('kind', ['sgd', 'rmsprop'])
def test_g17_twenty_steps_match_reference(kind, flat):
    from gated_gcrnns_amd.Modules.train_rnn import train_step
    from gated_gcrnns_amd.Utils.miscTools import batchTimeL1Loss, batchTimeMSELoss
    g = load_golden('g17_trace_' + kind)
    m = _g6_model(g)
    opt = _optimiser(kind, m.parameters(), flat, lr=float(g['lr']))
    assert kind != 'rmsprop' or float(g['alpha']) == 0.9
    x = torch.tensor(g['x'], device=DEV)
    y = torch.tensor(g['y'], device=DEV)
    losses, metrics = [], []
    for it in range(20):
        loss, yHat = train_step(m, batchTimeL1Loss, opt, x, y, 20)
        losses.append(float(loss))
        metrics.append(float(batchTimeMSELoss(yHat, y)))
    el, em = np.max(np.abs(np.array(losses) - g['loss'])), np.max(np.abs(np.array(metrics) - g['metric']))
    sd = m.state_dict()
    ep = max(np.max(np.abs(sd[k].cpu().numpy() - v)) for k, v in g['params20'].items())
    print('G17 %s flat=%s: max|loss - ref| = %.3g, max|metric - ref| = %.3g, max|param - ref| = %.3g' % (kind, flat, el, em, ep))
    assert g['loss'][-1] < 0.5 * g['loss'][0]                   # (the fixture's learning rate moves the loss)
    assert el <= 1e-9
    assert em <= 1e-8
    assert ep <= 1e-8


class _SampleOrder(object):
    """rng of MultipleModels whose epoch permutation is the sample order (the fixtures' batches are fixed)."""

    def permutation(self, n):
        return np.arange(n)


@pytest.mark.parametrize('flat', [True, False])
@pytest.mark.parametrize('name', ['adam_decay_p1', 'adam_decay_p2', 'rnnmlp_rmsprop_decay'])
def test_g17_decay_traces_through_multiple_models(name, flat, tmp_path):
    """MultipleModels itself with learningRateDecayRate / Period: the schedule is stepped at the top of every epoch (period 1: the first
    epoch already trains at lr * rate). Per-step loss and metric at G6's bounds; the learning rate in force at every step -- read back from
    the device scalar for the flat optimisers -- EQUALS the reference's."""
    import gated_gcrnns_amd.Modules.architectures as archit
    from gated_gcrnns_amd import optim
    from gated_gcrnns_amd.Modules.train_rnn import MultipleModels, TrainableModel
    from gated_gcrnns_amd.Utils.miscTools import batchTimeL1Loss, batchTimeMSELoss
    g = load_golden('g17_trace_' + name)
    if name.startswith('adam'):
        key, F = 'GCRNNMLP', 20
        m = _g6_model(g)
        opt = optim.make_trainer('ADAM', m.parameters(), float(g['lr0']), 0.9, 0.999, flat=flat)
    else:
        key, F = 'RNNMLP', 1
        m = archit.RNNforRegression(1, 1, 'tanh', [1], torch.nn.ReLU, g['S'][0], True).double()
        m.load_state_dict({k: torch.tensor(v) for k, v in g['params0'].items()})
        m = m.to(DEV)
        opt = optim.make_trainer('RMSprop', m.parameters(), float(g['lr0']), float(g['alpha']), 0.999, flat=flat)
    lrs = []

    def evaluate(yHat, y):                                      # called once per training step, behind the optimiser step
        lrs.append(_lr_of(opt))
        return batchTimeMSELoss(yHat, y)

    x = torch.tensor(g['x'][:, :, 0, :])                        # nTrain x T x N
    y = torch.tensor(g['y'][:, :, 0, :])
    out = MultipleModels({key: TrainableModel(m, batchTimeL1Loss, opt, key, str(tmp_path))}, x, y, None, None, int(g['epochs']),
                         int(g['batch']), 5, F, evaluate, validationInterval=0, rng=_SampleOrder(), rnnStateFeat=1,
                         learningRateDecayRate=float(g['rate']), learningRateDecayPeriod=int(g['period']))
    el = np.max(np.abs(np.array(out['lossTrain'][key]) - g['loss']))
    em = np.max(np.abs(np.array(out['evalTrain'][key]) - g['metric']))
    sd = m.state_dict()
    ep = max(np.max(np.abs(sd[k].cpu().numpy() - v)) for k, v in g['params_final'].items())
    print('G17 %s flat=%s: max|loss - ref| = %.3g, max|metric - ref| = %.3g, max|param - ref| = %.3g, lr %s' % (name, flat, el, em, ep, lrs))
    assert lrs == g['lr'].tolist()                              # equal, not close
    assert len(set(lrs)) > 1
    assert el <= 1e-9
    assert em <= 1e-8
    assert ep <= 1e-8


def _decay_under_capture(kind, two_graphs):
    from gated_gcrnns_amd import optim
    from gated_gcrnns_amd.Modules.train_rnn import train_step, GraphedTrainStep
    from gated_gcrnns_amd.Utils.miscTools import batchTimeL1Loss
    g = load_golden('g6_trace_GCRNNMLP')
    x = torch.tensor(g['x'], device=DEV)
    y = torch.tensor(g['y'], device=DEV)
    me, mg = _g6_model(g), _g6_model(g)
    oe, og = _optimiser(kind, me.parameters(), True), _optimiser(kind, mg.parameters(), True)
    se, sg = optim.StepDecay(oe, 2, 0.5), optim.StepDecay(og, 2, 0.5)
    stepper = GraphedTrainStep(mg, batchTimeL1Loss, og, x, y, 20, sync=og.sync if two_graphs else None)   # 3 eager warm-up steps inside
    assert (stepper.graph_step is not None) == two_graphs
    for _ in range(3):
        train_step(me, batchTimeL1Loss, oe, x, y, 20)
    lr0 = og.lr
    for it in range(8):
        if it % 2 == 0:                                         # "epochs" of two steps at lr0, lr0/2, lr0/2, lr0/4
            se.step()
            sg.step()
        le, _ = train_step(me, batchTimeL1Loss, oe, x, y, 20)
        lg, _ = stepper(x, y)
        assert float(le) == float(lg), (kind, it, float(le), float(lg))
    assert og.lr == oe.lr == lr0 * 0.25
    for p, q in zip(me.parameters(), mg.parameters()):
        assert torch.equal(p, q)
    # and the decayed steps are not the undecayed ones: the same replays without a schedule end somewhere else
    mu = _g6_model(g)
    ou = _optimiser(kind, mu.parameters(), True)
    for _ in range(11):
        train_step(mu, batchTimeL1Loss, ou, x, y, 20)
    assert not all(torch.equal(p, q) for p, q in zip(mu.parameters(), mg.parameters()))


@pytest.mark.parametrize('kind', ['sgd', 'rmsprop', 'adam'])
def test_decay_reaches_a_captured_step(kind):
    """GraphedTrainStep (ONE graph) with each flat optimiser, StepDecay.step() between replays: the learning rate is a device scalar that the
    captured kernel reads, so the replayed trace is bit-identical to the eager trace of the same optimiser and schedule."""
    _decay_under_capture(kind, two_graphs=False)


def test_decay_reaches_a_captured_step_two_graph_form():
    """The multi-rank form (sync=opt.sync, world 1): [zero_grad .. BPTT] and [Adam step] as two graphs around the flat all-reduce."""
    _decay_under_capture('adam', two_graphs=True)


@pytest.mark.parametrize('dt', [torch.float32, torch.float64])
def test_adam_with_device_lr_is_flat_adam_bit_for_bit(dt):
    from gated_gcrnns_amd.Modules.train_rnn import train_step
    from gated_gcrnns_amd.Utils.miscTools import batchTimeL1Loss
    from gated_gcrnns_amd.optim import FlatAdam
    g = load_golden('g6_trace_GCRNNMLP')
    x = torch.tensor(g['x'], device=DEV, dtype=dt)
    y = torch.tensor(g['y'], device=DEV, dtype=dt)
    ma, mb = _g6_model(g, dt), _g6_model(g, dt)
    oa, ob = FlatAdam(ma.parameters(), lr=1e-3, betas=(0.9, 0.999)), FlatAdam(mb.parameters(), lr=1e-3, betas=(0.9, 0.999), device_lr=True)
    assert oa.lr_dev is None and ob.lr_dev is not None
    for it in range(20):
        la, _ = train_step(ma, batchTimeL1Loss, oa, x, y, 20)
        lb, _ = train_step(mb, batchTimeL1Loss, ob, x, y, 20)
        assert float(la) == float(lb), it
    assert torch.equal(oa.flat_p, ob.flat_p) and torch.equal(oa.m, ob.m) and torch.equal(oa.v, ob.v)
    assert int(ob.step_dev) == 20 and float(ob.m.abs().max()) > 0


@pytest.mark.parametrize('kind', ['sgd', 'rmsprop', 'adam'])
def test_fp32_flat_against_torch_optim(kind):
    """fp32 parameters: each flat optimiser against its torch.optim counterpart on the same model, 10 steps, loss within the project's fp32 bound."""
    from gated_gcrnns_amd.Modules.train_rnn import train_step
    from gated_gcrnns_amd.Utils.miscTools import batchTimeL1Loss
    g = load_golden('g6_trace_GCRNNMLP')
    x = torch.tensor(g['x'], device=DEV, dtype=torch.float32)
    y = torch.tensor(g['y'], device=DEV, dtype=torch.float32)
    mf, mt = _g6_model(g, torch.float32), _g6_model(g, torch.float32)
    of, ot = _optimiser(kind, mf.parameters(), True), _optimiser(kind, mt.parameters(), False)
    assert of.flat_p.dtype == torch.float32
    errs = []
    for it in range(10):
        lf, _ = train_step(mf, batchTimeL1Loss, of, x, y, 20)
        lt, _ = train_step(mt, batchTimeL1Loss, ot, x, y, 20)
        errs.append(abs(float(lf) - float(lt)))
    print('fp32 %s: max|loss flat - loss torch| = %.3g' % (kind, max(errs)))
    assert max(errs) <= 1e-5, errs


def _kernel_launches(fn):
    """Device events of one call by kernel name (as tests/test_rnn_baseline.py counts launches)."""
    from torch.profiler import profile, ProfilerActivity
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return collections.Counter(e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


OURS = ('sgd_flat', 'rmsprop_flat', 'adam_flat', 'adam_tick')


def _ours(counter):
    return {k: v for k, v in counter.items() if any(o in k for o in OURS)}


def test_launches_per_step():
    from gated_gcrnns_amd.optim import FlatAdam
    g = load_golden('g6_trace_GCRNNMLP')
    counts = {}
    for kind in ('sgd', 'rmsprop', 'adam', 'adam_host'):
        m = _g6_model(g)
        opt = FlatAdam(m.parameters(), lr=1e-3) if kind == 'adam_host' else _optimiser(kind, m.parameters(), True)
        opt.sync.flat.normal_()
        opt.step()                                              # (first call outside the profile)
        every = _kernel_launches(opt.step)
        counts[kind] = _ours(every)
        assert sum(every.values()) == sum(counts[kind].values()), every           # a step launches nothing but the library's kernels
        if kind != 'adam_host':
            filled = _kernel_launches(lambda: opt.set_lr(5e-4))
            assert not _ours(filled) and not any('gcrnn' in k for k in filled), filled      # a fill of torch's, no kernel of ours
            assert opt.lr == 5e-4
    print(counts)
    assert sum(counts['sgd'].values()) == 1 and all('sgd_flat' in k for k in counts['sgd'])
    assert sum(counts['rmsprop'].values()) == 1 and all('rmsprop_flat' in k for k in counts['rmsprop'])
    assert sum(counts['adam'].values()) == sum(counts['adam_host'].values()) == 2
    assert any('adam_flat_dlr' in k for k in counts['adam']) and not any('adam_flat_dlr' in k for k in counts['adam_host'])


def test_argument_errors_of_the_new_entry_points():
    """Null pointers, n <= 0 and a dtype that is neither F32 nor F64 return the status codes gcrnn_adam_flat returns, before any launch."""
    from gated_gcrnns_amd import _lib
    L = _lib.lib
    n = 16
    p, gr, m, v = (torch.zeros(n, dtype=torch.float64, device=DEV) for _ in range(4))
    lr = torch.full((1,), 1e-3, dtype=torch.float64, device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    P = lambda t: C.c_void_p(t.data_ptr())
    null_code = L.gcrnn_adam_flat(_lib.F64, None, P(gr), P(m), P(v), n, 1e-3, 0.9, 0.999, 1e-8, 1.0, P(step), None)
    shape_code = L.gcrnn_adam_flat(_lib.F64, P(p), P(gr), P(m), P(v), 0, 1e-3, 0.9, 0.999, 1e-8, 1.0, P(step), None)
    assert (null_code, shape_code) == (3, 2)
    dtype_code = 1                                              # GCRNN_ERR_BAD_DTYPE (include/gcrnn.h)

    q = lambda t: P(t) if t is not None else None

    def sgd(dt=_lib.F64, p_=p, g_=gr, n_=n, lr_=lr):
        return L.gcrnn_sgd_flat(dt, q(p_), q(g_), n_, q(lr_), 1.0, None)

    def rms(dt=_lib.F64, p_=p, g_=gr, v_=v, n_=n, lr_=lr):
        return L.gcrnn_rmsprop_flat(dt, q(p_), q(g_), q(v_), n_, q(lr_), 0.9, 1e-8, 1.0, None)

    def adam(dt=_lib.F64, p_=p, g_=gr, m_=m, v_=v, n_=n, lr_=lr, s_=step):
        return L.gcrnn_adam_flat_dlr(dt, q(p_), q(g_), q(m_), q(v_), n_, q(lr_), 0.9, 0.999, 1e-8, 1.0, q(s_), None)

    for fn, ptrs in ((sgd, ('p_', 'g_', 'lr_')), (rms, ('p_', 'g_', 'v_', 'lr_')), (adam, ('p_', 'g_', 'm_', 'v_', 'lr_', 's_'))):
        for k in ptrs:
            assert fn(**{k: None}) == null_code, (fn.__name__, k)
        assert fn(n_=0) == shape_code and fn(n_=-5) == shape_code, fn.__name__
        assert fn(dt=_lib.BF16) == dtype_code and fn(dt=7) == dtype_code and fn(dt=-1) == dtype_code, fn.__name__
    torch.cuda.synchronize()
    assert int(step) == 0 and float(p.abs().max()) == 0.0      # nothing was launched
    with pytest.raises(_lib.GcrnnError):
        _lib.check(sgd(n_=0), 'sgd_flat')


@pytest.mark.parametrize('kind', ['sgd', 'rmsprop', 'adam'])
def test_checkpoint_restores_optimiser_and_schedule(kind, tmp_path):
    """TrainableModel.save / load go through the optimiser's state_dict: a checkpoint of each new optimiser with a schedule attached restores
    parameters, moments, learning rate and the schedule's count, and training continues identically."""
    from gated_gcrnns_amd import optim
    from gated_gcrnns_amd.Modules.train_rnn import train_step, TrainableModel
    from gated_gcrnns_amd.Utils.miscTools import batchTimeL1Loss
    g = load_golden('g6_trace_GCRNNMLP')
    x = torch.tensor(g['x'], device=DEV)
    y = torch.tensor(g['y'], device=DEV)

    def make():
        m = _g6_model(g)
        opt = _optimiser(kind, m.parameters(), True)
        return m, opt, optim.StepDecay(opt, 2, 0.5), TrainableModel(m, batchTimeL1Loss, opt, 'GCRNNMLP', str(tmp_path))

    def epochs(m, opt, sched, n):
        out = []
        for _ in range(n):
            sched.step()
            out += [float(train_step(m, batchTimeL1Loss, opt, x, y, 20)[0]) for _ in range(2)]
        return out

    ma, oa, sa, ta = make()
    epochs(ma, oa, sa, 3)
    ta.save('Last')
    want = epochs(ma, oa, sa, 3)
    mb, ob, sb, tb = make()
    tb.load('Last')
    assert sb.epoch == 3 and ob.lr == _lr_of(_optimiser(kind, _g6_model(g).parameters(), True)) * 0.5
    got = epochs(mb, ob, sb, 3)
    assert got == want
    assert oa.lr == ob.lr and torch.equal(oa.flat_p, ob.flat_p)


@pytest.mark.parametrize('how', ['flat', 'torch'])
def test_examples_run_with_the_new_trainers(how):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples'))
    import kstep_prediction
    import epicenter_estimation
    old = torch.get_default_dtype()
    try:
        for extra in (['--trainer', 'SGD'], ['--trainer', 'RMSprop', '--lr-decay-rate', '0.9', '--lr-decay-period', '1']):
            res = kstep_prediction.main(['--models', 'GCRNNMLP,RNNMLP', '--ntrain', '200', '--epochs', '2', '--nodes', '40', '--optim', how] + extra)
            assert set(res) == {'GCRNNMLP', 'RNNMLP'} and all(np.isfinite(r['score']) for r in res.values()), (how, extra, res)
            assert all(np.all(np.isfinite(r['loss'])) for r in res.values())
            res = epicenter_estimation.main(['--models', 'GCRNNMLP', '--steps', '6', '--steps-per-epoch', '2', '--seq', '20', '--optim', how] + extra)
            assert 0.0 <= res['accuracy'] <= 1.0 and np.all(np.isfinite(res['loss'])), (how, extra, res)
    finally:
        torch.set_default_dtype(old)
