"""CPU: the drivers' trainers (`trainer = 'SGD' | 'ADAM' | 'RMSprop'`, kStepPredGRNNs.py:158-161, 706-715) and learning-rate decay
(Modules/train_rnn.py:85-91, 149-155, 197-200) at the Python surface: the flat optimisers' torch branch against torch.optim, StepDecay
against torch's StepLR, make_trainer's dispatch and MultipleModels' keywords. The HIP kernels are tested in test_trainers.py."""
import inspect

import numpy as np
import pytest
import torch

from gated_gcrnns_amd import optim
from gated_gcrnns_amd.Modules import train_rnn

SHAPES = [(3, 7), (5,), (1,), (2, 3, 5), (13, 1)]          # 21 + 5 + 1 + 30 + 13 = 70 elements, no power of two anywhere


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, dtype=torch.float64, generator=g)) for s in SHAPES]


CASES = {
    'sgd': (lambda p: optim.FlatSGD(p, lr=0.05), lambda p: torch.optim.SGD(p, lr=0.05)),
    'rmsprop': (lambda p: optim.FlatRMSprop(p, lr=0.01, alpha=0.9), lambda p: torch.optim.RMSprop(p, lr=0.01, alpha=0.9)),
    'adam_dlr': (lambda p: optim.FlatAdam(p, lr=0.01, betas=(0.8, 0.99), device_lr=True),
                 lambda p: torch.optim.Adam(p, lr=0.01, betas=(0.8, 0.99))),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_flat_optimiser_matches_torch_optim_on_cpu(name):
    """10 steps on random fp64 gradients with grad_scale != 1: same element-wise arithmetic in the same order -> 1e-12."""
    flat_of, torch_of = CASES[name]
    pf, pt = _params(1), _params(1)
    of, ot = flat_of(pf), torch_of(pt)
    g = torch.Generator().manual_seed(2)
    scale = 0.37
    for it in range(10):
        of.zero_grad()
        for a, b in zip(pf, pt):
            gr = torch.randn(*a.shape, dtype=torch.float64, generator=g)
            a.grad.add_(gr)                                       # the flat optimiser's gradients are views of one flat buffer
            b.grad = gr * scale
        of.step(grad_scale=scale)
        ot.step()
        err = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(pf, pt))
        print('%s step %d max|flat - torch| = %.3g' % (name, it, err))
        assert err <= 1e-12, (name, it, err)
    assert all(a.data_ptr() == of.flat_p.data_ptr() + off * 8 for a, off in zip(pf, np.cumsum([0] + [int(np.prod(s)) for s in SHAPES])))


@pytest.mark.parametrize('name', sorted(CASES))
def test_state_dict_round_trip_continues_identically(name):
    flat_of, _ = CASES[name]
    g = torch.Generator().manual_seed(3)
    grads = [[torch.randn(*s, dtype=torch.float64, generator=g) for s in SHAPES] for _ in range(6)]

    def run(opt, ps, its):
        for it in its:
            opt.zero_grad()
            for p, gr in zip(ps, grads[it]):
                p.grad.add_(gr)
            opt.step()

    pa = _params(4)
    oa = flat_of(pa)
    sa = optim.StepDecay(oa, 2, 0.5)
    for it in range(3):
        sa.step()
        run(oa, pa, [it])
    sd = oa.state_dict()
    assert sd['schedule'] == {'epoch': 3, 'period': 2, 'rate': 0.5} and sd['lr'] == oa.lr
    pb = _params(5)
    ob = flat_of(pb)
    sb = optim.StepDecay(ob, 1, 0.1)
    ob.load_state_dict(sd)
    assert sb.epoch == 3 and sb.period == 2 and ob.lr == oa.lr
    for it in range(3, 6):
        sa.step(); sb.step()
        run(oa, pa, [it]); run(ob, pb, [it])
        assert oa.lr == ob.lr
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)


@pytest.mark.parametrize('period', [1, 2, 3])
def test_step_decay_equals_torch_steplr(period):
    """Learning rates EQUAL torch's, not close: the recursive product lr *= rate, not lr0 * rate ** (epoch // period)."""
    pf, pt = _params(1), _params(1)
    of, ot = optim.FlatSGD(pf, lr=1e-3), torch.optim.SGD(pt, lr=1e-3)
    sf, st = optim.StepDecay(of, period, 0.9), optim.StepDecay(ot, period, 0.9)
    assert type(sf) is optim.StepDecay and type(st) is torch.optim.lr_scheduler.StepLR
    mid = None
    seq = []
    for epoch in range(10):
        ot.step()                                  # (keeps torch's "scheduler before optimiser" warning out of the test)
        sf.step(); st.step()
        assert of.lr == ot.param_groups[0]['lr'] == st.get_last_lr()[0] == sf.get_last_lr()[0], (epoch, of.lr, ot.param_groups[0]['lr'])
        seq.append(of.lr)
        if epoch == 4:
            mid = (sf.state_dict(), of.lr)
    assert seq[-1] < seq[0]
    o2 = optim.FlatSGD(_params(1), lr=123.0)
    s2 = optim.StepDecay(o2, 7, 0.5)
    s2.load_state_dict(mid[0])
    o2.set_lr(mid[1])
    for epoch in range(5, 10):
        s2.step()
        assert o2.lr == seq[epoch]


def test_set_lr_and_device_lr_flag():
    o = optim.FlatAdam(_params(1), lr=1e-3)
    assert o.lr_dev is None and o.lr == 1e-3
    with pytest.raises(RuntimeError, match='launch argument'):
        o.set_lr(1e-4)
    with pytest.raises(RuntimeError, match='launch argument'):
        optim.StepDecay(o, 1, 0.9)
    o.lr = 2e-3                                    # the host value stays an attribute, as before
    assert o.lr == 2e-3
    for o in (optim.FlatAdam(_params(1), lr=1e-3, device_lr=True), optim.FlatSGD(_params(1), lr=1e-3), optim.FlatRMSprop(_params(1), lr=1e-3)):
        assert o.lr_dev.dtype == torch.float64 and o.lr_dev.numel() == 1 and o.lr == 1e-3
        o.set_lr(0.3)
        assert o.lr == 0.3 and float(o.lr_dev) == 0.3


@pytest.mark.parametrize('flat', [True, False])
def test_make_trainer(flat):
    mk = lambda name: optim.make_trainer(name, _params(1), 2e-3, 0.8, 0.95, flat=flat)
    a, s, r = mk('ADAM'), mk('SGD'), mk('RMSprop')
    if flat:
        assert type(a) is optim.FlatAdam and a.lr_dev is not None and a.lr == 2e-3 and a.betas == (0.8, 0.95) and a.eps == 1e-8
        assert type(s) is optim.FlatSGD and s.lr == 2e-3
        assert type(r) is optim.FlatRMSprop and r.lr == 2e-3 and r.alpha == 0.8 and r.eps == 1e-8
    else:
        assert type(a) is torch.optim.Adam and a.defaults['lr'] == 2e-3 and tuple(a.defaults['betas']) == (0.8, 0.95)
        assert type(s) is torch.optim.SGD and s.defaults['lr'] == 2e-3 and s.defaults['momentum'] == 0 and s.defaults['weight_decay'] == 0
        assert type(r) is torch.optim.RMSprop and r.defaults['lr'] == 2e-3 and r.defaults['alpha'] == 0.8 and r.defaults['eps'] == 1e-8
        assert r.defaults['momentum'] == 0 and not r.defaults['centered']
    with pytest.raises(ValueError, match="'SGD', 'ADAM', 'RMSprop'"):
        mk('Adam')


def test_multiple_models_has_the_decay_keywords():
    ps = inspect.signature(train_rnn.MultipleModels).parameters
    names = list(ps)
    assert ps['learningRateDecayRate'].default is None and ps['learningRateDecayPeriod'].default is None
    assert names.index('rnnStateFeat') < names.index('learningRateDecayRate') < names.index('learningRateDecayPeriod')
    assert ps['rnnStateFeat'].default is None
