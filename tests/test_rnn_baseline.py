"""GPU: the drivers' plain-RNN baselines on the recurrence kernels (gcrnn_rnn.hip) -- the G16 fixtures of the reference's autograd,
edge shapes against an fp64 torch composition, the large shape in fp32, the composed path one step outside the envelope,
bit-identical gradients, launch counts independent of T, the training harness, the reference's Adam trace and both examples."""
import collections

import numpy as np
import pytest
import torch

from conftest import load_golden
import gated_gcrnns_amd.Modules.architectures as archit
from gated_gcrnns_amd import ops
from gated_gcrnns_amd.Modules import train_rnn
from gated_gcrnns_amd.Utils import miscTools

pytestmark = pytest.mark.gpu
DEV = 'cuda'


class _CountingLib(object):
    """ops.lib with a call counter on the gcrnn_rnn_* compute entry points (the queries pass through)."""

    def __init__(self, lib):
        self._lib = lib
        self.calls = collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith('gcrnn_rnn_') or name.endswith(('_supported', '_slots')):
            return fn

        def counted(*a):
            self.calls[name] += 1
            return fn(*a)
        return counted


@pytest.fixture
def spy(monkeypatch):
    s = _CountingLib(ops.lib)
    monkeypatch.setattr(ops, 'lib', s)
    return s


@pytest.fixture
def no_fallback(monkeypatch):
    def composed(*a, **k):
        raise AssertionError('composed fallback taken')
    monkeypatch.setattr(ops, '_rnn_sequence_composed', composed)


def torch_rnn(x, h0, wi, wh, bi, bh, act):
    """fp64 reference: h_t = act(W_ih x_t + b_ih + W_hh h_{t-1} + b_hh), step by step (written here, independent of ops)."""
    f = torch.tanh if act == 'tanh' else torch.relu
    h, out = h0, []
    for t in range(x.shape[1]):
        z = x[:, t] @ wi.t() + h @ wh.t()
        if bi is not None:
            z = z + bi + bh
        h = f(z)
        out.append(h)
    return torch.stack(out, 1)


def _err(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).abs().max()) / max(1e-300, float(ref.abs().max()))


def _g16_model(name, g):
    S = g['S'][0]
    if name == 'g16_rnn_reg_kstep':
        return archit.RNNforRegression(1, 1, 'tanh', [1], torch.nn.ReLU, S, True)
    if name == 'g16_rnn_cls_quake':
        return archit.RNNforClassification(1, 21, 'tanh', [11], torch.nn.ReLU, S, True)
    return archit.RNNforRegression(2, 8, 'relu', [6, 1], torch.nn.ReLU, S, False, finalNonlinearity=torch.nn.ReLU)


@pytest.mark.parametrize('dt,tol', [(torch.float64, 1e-11), (torch.float32, 1e-5)])
@pytest.mark.parametrize('name', ['g16_rnn_reg_kstep', 'g16_rnn_cls_quake', 'g16_rnn_reg_deep'])
def test_g16_fixture_forward_and_gradients(name, dt, tol, spy, no_fallback):
    g = load_golden(name)
    m = _g16_model(name, g).double()
    m.load_state_dict({k: torch.tensor(v) for k, v in g['params'].items()})
    m = m.to(DEV).to(dt)
    x = torch.tensor(g['x'], dtype=dt, device=DEV, requires_grad=True)
    h0 = torch.tensor(g['h0'], dtype=dt, device=DEV, requires_grad=True)
    y = m(x, h0, h0)
    (y * torch.tensor(g['R'], dtype=dt, device=DEV)).sum().backward()
    assert spy.calls == {'gcrnn_rnn_forward': 1, 'gcrnn_rnn_backward': 1}, dict(spy.calls)
    checks = [('y', y, g['y']), ('x', x.grad, g['grad_x']), ('h0', h0.grad, g['grad_h0'])]
    checks += [(k, p.grad, g['grads'][k]) for k, p in m.named_parameters()]
    assert sorted(k for k, _ in m.named_parameters()) == sorted(g['grads'])
    for what, a, ref in checks:
        err = _err(a, torch.tensor(ref))
        assert err <= tol, '%s %s %s: rel err %g' % (name, dt, what, err)


def _case(B, T, D, Fh, act, bias, dt, seed, shift=0.0):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    s = 1.0 / np.sqrt(max(D, Fh))
    x, h0 = r(B, T, D), 0.5 * r(B, Fh)
    wi, wh = s * r(Fh, D), (1.0 / np.sqrt(Fh)) * r(Fh, Fh)
    bi = (0.3 * r(Fh) + shift) if bias else None
    bh = (0.3 * r(Fh) + shift) if bias else None
    ts = [t.to(DEV).requires_grad_(True) if t is not None else None for t in (x, h0, wi, wh, bi, bh)]
    ks = [t.detach().to(dt).requires_grad_(True) if t is not None else None for t in ts]
    R = r(B, T, Fh).to(DEV)
    return ts, ks, R


def _compare(ts, ks, R, act, tol, what):
    ref = torch_rnn(*ts, act)
    (ref * R).sum().backward()
    H = ops.rnn_sequence(*ks, act)
    (H * R.to(H.dtype)).sum().backward()
    assert _err(H, ref) <= tol, '%s H: %g' % (what, _err(H, ref))
    for i, nm in enumerate(('x', 'h0', 'w_ih', 'w_hh', 'b_ih', 'b_hh')):
        if ts[i] is not None:
            e = _err(ks[i].grad, ts[i].grad)
            assert e <= tol, '%s d%s: %g' % (what, nm, e)


EDGES = [  # B, T, D, F_h, act, bias, shift
    (5, 7, 13, 1, 'tanh', True, 0.0),      # F_h = 1 (the k-step driver's state)
    (6, 9, 31, 17, 'tanh', True, 0.0),     # F_h between the register tiles, D not a multiple of 4
    (4, 6, 40, 64, 'tanh', True, 0.0),     # F_h = 64, the envelope's maximum
    (3, 1, 10, 8, 'tanh', True, 0.0),      # T = 1
    (1, 12, 9, 5, 'relu', True, 0.0),      # B = 1
    (67, 3, 22, 9, 'tanh', False, 0.0),    # B*T not a multiple of the 64-row tiles, no bias
    (7, 10, 15, 12, 'relu', True, -1.5),   # ReLU with mostly negative pre-activations
]


@pytest.mark.parametrize('dt,tol', [(torch.float64, 1e-11), (torch.float32, 1e-5)])
@pytest.mark.parametrize('case', EDGES, ids=['fh1', 'fh17_d31', 'fh64', 't1', 'b1', 'b67_nobias', 'relu_neg'])
def test_edge_shapes_against_torch_fp64(case, dt, tol, spy, no_fallback):
    B, T, D, Fh, act, bias, shift = case
    ts, ks, R = _case(B, T, D, Fh, act, bias, dt, seed=B * 1000 + T * 10 + Fh, shift=shift)
    _compare(ts, ks, R, act, tol, str(case))
    assert spy.calls == {'gcrnn_rnn_forward': 1, 'gcrnn_rnn_backward': 1}, dict(spy.calls)


def test_large_shape_fp32(spy, no_fallback):
    ts, ks, R = _case(256, 32, 1000, 64, 'tanh', True, torch.float32, seed=7)
    _compare(ts, ks, R, 'tanh', 1e-5, 'large')
    assert spy.calls == {'gcrnn_rnn_forward': 1, 'gcrnn_rnn_backward': 1}, dict(spy.calls)


@pytest.mark.parametrize('dt,tol', [(torch.float64, 1e-11), (torch.float32, 1e-5)])
def test_one_step_outside_envelope_takes_composed_path(dt, tol, spy):
    assert not ops.rnn_supported(dt, 3, 4, 10, 65)
    ts, ks, R = _case(3, 4, 10, 65, 'tanh', True, dt, seed=65)
    _compare(ts, ks, R, 'tanh', tol, 'F_h = 65')
    assert not spy.calls


def test_gradients_bit_identical_between_runs():
    ts, ks, R = _case(100, 20, 59, 21, 'tanh', True, torch.float32, seed=3)
    grads = []
    for _ in range(2):
        for k in ks:
            k.grad = None
        (ops.rnn_sequence(*ks, 'tanh') * R.float()).sum().backward()
        grads.append([k.grad.clone() for k in ks])
    for a, b in zip(*grads):
        assert torch.equal(a, b)


def _kernel_launches(fn):
    from torch.profiler import profile, ProfilerActivity
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return collections.Counter(e.name.split('<')[0].split('(')[0].replace('void ', '').strip() for e in prof.events()
                               if e.device_type == torch.autograd.DeviceType.CUDA and 'rnn_' in e.name)


def test_launch_counts_independent_of_T():
    counts = {}
    for T in (5, 200):
        ts, ks, R = _case(100, T, 80, 1, 'tanh', True, torch.float32, seed=T)
        H = ops.rnn_sequence(*ks, 'tanh')
        fwd = _kernel_launches(lambda: ops.rnn_sequence(*ks, 'tanh'))
        bwd = _kernel_launches(lambda: (H * R.float()).sum().backward())
        counts[T] = (fwd, bwd)
    assert counts[5] == counts[200], counts
    fwd, bwd = counts[5]
    assert 1 <= sum(fwd.values()) <= 2 and 1 <= sum(bwd.values()) <= 3, counts


def _kstep_data(seed, n, T, N):
    rng = np.random.default_rng(seed)
    return torch.tensor(rng.standard_normal((n, T, N))), torch.tensor(rng.standard_normal((n, T, N)))


def test_multiple_models_trains_rnnmlp_next_to_gcrnnmlp(tmp_path):
    torch.manual_seed(0)
    N, T = 20, 5
    S = np.eye(N, k=1) + np.eye(N, k=-1)
    S = S / np.max(np.abs(np.linalg.eigvalsh(S)))
    gm = archit.GatedGCRNNforRegression(1, 4, 2, 2, torch.tanh, torch.nn.ReLU, [1], S, True, False, None, 'multipMlp').to(DEV).double()
    rm = archit.RNNforRegression(1, 3, 'tanh', [1], torch.nn.ReLU, S, True).to(DEV).double()
    models = {name: train_rnn.TrainableModel(m, miscTools.batchTimeL1Loss, torch.optim.Adam(m.parameters(), lr=1e-3), name,
                                             str(tmp_path)) for name, m in (('GCRNNMLP', gm), ('RNNMLP', rm))}
    xT, yT = _kstep_data(1, 40, T, N)
    xV, yV = _kstep_data(2, 10, T, N)
    p0 = rm.RNN.weight_ih_l0.detach().clone()
    out = train_rnn.MultipleModels(models, xT, yT, xV, yV, 1, 10, T, 4, miscTools.batchTimeL1Loss, validationInterval=2,
                                   rng=np.random.RandomState(0))
    for name in models:
        assert len(out['lossTrain'][name]) == 4 and np.all(np.isfinite(out['lossTrain'][name])), name
        assert len(out['evalValid'][name]) == 2 and np.isfinite(out['bestScore'][name]), name
    assert not torch.equal(p0, rm.RNN.weight_ih_l0.detach())
    assert (tmp_path / 'savedModels' / 'RNNMLPArchitBest.ckpt').exists()


def test_adam_trace_reproduces_reference(no_fallback):
    g = load_golden('g16_trace_rnnmlp')
    m = archit.RNNforRegression(1, 1, 'tanh', [1], torch.nn.ReLU, g['S'][0], True).double()
    m.load_state_dict({k: torch.tensor(v) for k, v in g['params0'].items()})
    m = m.to(DEV)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, betas=(0.9, 0.999))
    fwd = train_rnn._rnn_forward(1)
    losses = []
    for it in range(g['x'].shape[0]):
        x = torch.tensor(g['x'][it], device=DEV)
        y = torch.tensor(g['y'][it], device=DEV)
        loss, _ = train_rnn.train_step(m, miscTools.batchTimeL1Loss, opt, x, y, 1, forward=fwd)
        losses.append(float(loss))
    assert np.max(np.abs(np.array(losses) - g['loss'])) <= 1e-9 * max(1.0, np.max(np.abs(g['loss']))), (losses, g['loss'])
    for k, v in m.state_dict().items():
        assert _err(v, torch.tensor(g['params10'][k])) <= 1e-9, k


def test_examples_run_rnnmlp():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples'))
    import kstep_prediction
    import epicenter_estimation
    old = torch.get_default_dtype()
    try:
        res = kstep_prediction.main(['--models', 'GCRNNMLP,RNNMLP', '--ntrain', '200', '--epochs', '1', '--nodes', '40'])
        assert set(res) == {'GCRNNMLP', 'RNNMLP'} and all(np.isfinite(r['score']) for r in res.values())
        res = epicenter_estimation.main(['--models', 'RNNMLP', '--steps', '4', '--seq', '20'])
        assert 0.0 <= res['accuracy'] <= 1.0 and np.all(np.isfinite(res['loss']))
    finally:
        torch.set_default_dtype(old)
