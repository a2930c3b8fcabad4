"""CPU: the plain-RNN baselines (RNNforRegression / RNNforClassification) mirror the reference's constructor, argument errors,
state_dict keys and seeded initialisation (G16 fixtures); a forward on CPU tensors raises; the gcrnn_rnn_* entry points are
exported and reject bad arguments on the host, before any launch."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from conftest import load_golden
import gated_gcrnns_amd.Modules.architectures as archit
from gated_gcrnns_amd import _lib, ops
from gated_gcrnns_amd.Modules import train_rnn

SIGNATURE = ['inFeatures', 'stateFeatures', 'stateNonlinearity', 'dimLayersMLP', 'outputNonlinearity', 'GSO', 'bias',
             'finalNonlinearity']
RNN_SYMBOLS = ['gcrnn_rnn_supported', 'gcrnn_rnn_wgrad_slots', 'gcrnn_rnn_forward', 'gcrnn_rnn_backward']


def _model(name, g):
    S = g['S'][0]
    if name == 'g16_rnn_reg_kstep':
        return archit.RNNforRegression(1, 1, 'tanh', [1], torch.nn.ReLU, S, True)
    if name == 'g16_rnn_cls_quake':
        return archit.RNNforClassification(1, 21, 'tanh', [11], torch.nn.ReLU, S, True)
    return archit.RNNforRegression(2, 8, 'relu', [6, 1], torch.nn.ReLU, S, False, finalNonlinearity=torch.nn.ReLU)


@pytest.fixture
def fp64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)          # the fixtures were drawn in the drivers' default dtype
    yield
    torch.set_default_dtype(old)


@pytest.mark.parametrize('cls', [archit.RNNforRegression, archit.RNNforClassification])
def test_constructor_signature_matches_reference(cls):
    params = inspect.signature(cls.__init__).parameters
    assert list(params)[1:] == SIGNATURE
    assert params['finalNonlinearity'].default is None
    assert list(inspect.signature(cls.forward).parameters) == ['self', 'x', 'h0', 'c0']


@pytest.mark.parametrize('cls', [archit.RNNforRegression, archit.RNNforClassification])
def test_argument_errors_match_reference(cls):
    S = np.eye(5)
    with pytest.raises(ValueError, match="Unknown nonlinearity 'sigmoid'"):
        cls(1, 4, 'sigmoid', [1], torch.nn.ReLU, S, True)
    with pytest.raises(ValueError, match='hidden_size must be greater than zero'):
        cls(1, 0, 'tanh', [1], torch.nn.ReLU, S, True)
    with pytest.raises(TypeError):
        cls(1, 4.0, 'tanh', [1], torch.nn.ReLU, S, True)
    with pytest.raises(AssertionError):
        cls(1, 4, 'tanh', [1], torch.nn.ReLU, np.ones((5, 4)), True)             # not square
    with pytest.raises(AssertionError):
        cls(1, 4, 'tanh', [1], torch.nn.ReLU, np.ones((2, 5, 4)), True)
    with pytest.raises(AssertionError):
        cls(1, 4, 'tanh', [1], torch.nn.ReLU, np.ones(5), True)


@pytest.mark.parametrize('name', ['g16_rnn_reg_kstep', 'g16_rnn_cls_quake', 'g16_rnn_reg_deep'])
def test_state_dict_keys_and_seeded_init_equal_reference(name, fp64_default):
    g = load_golden(name)
    torch.manual_seed(int(g['seed']))
    m = _model(name, g)
    sd = m.state_dict()
    assert sorted(sd) == sorted(g['params'])
    for k, v in sd.items():
        assert v.dtype == torch.float64 and tuple(v.shape) == g['params'][k].shape, k
        assert np.array_equal(v.numpy(), g['params'][k]), k
    if name == 'g16_rnn_reg_deep':
        assert not any('bias' in k for k in sd)
        assert [type(l) for l in m.outputNN] == [torch.nn.Linear, torch.nn.ReLU, torch.nn.Linear, torch.nn.ReLU]
        assert m.outputNN[2].out_features == 30
    assert 'S' not in sd and m.S.shape == (1, g['S'].shape[1], g['S'].shape[2])


def test_trace_fixture_initial_parameters(fp64_default):
    g = load_golden('g16_trace_rnnmlp')
    torch.manual_seed(int(g['seed']))
    m = archit.RNNforRegression(1, 1, 'tanh', [1], torch.nn.ReLU, g['S'][0], True)
    for k, v in m.state_dict().items():
        assert np.array_equal(v.numpy(), g['params0'][k]), k


def test_final_nonlinearity_on_empty_mlp():
    m = archit.RNNforClassification(1, 3, 'tanh', [], torch.nn.ReLU, np.eye(4), True, finalNonlinearity=torch.nn.Sigmoid)
    assert [type(l) for l in m.outputNN] == [torch.nn.Sigmoid]


def test_forward_on_cpu_raises():
    m = archit.RNNforRegression(1, 3, 'tanh', [1], torch.nn.ReLU, np.eye(4), True).float()
    x, h0 = torch.zeros(2, 3, 1, 4), torch.zeros(2, 3)
    with pytest.raises(_lib.GcrnnError, match='no CPU path'):
        m(x, h0, h0)
    with pytest.raises(_lib.GcrnnError):
        ops.rnn_sequence(x.view(2, 3, 4), h0, m.RNN.weight_ih_l0, m.RNN.weight_hh_l0, None, None, 'tanh')


def test_harness_no_longer_rejects_rnn_models():
    assert 'NotImplementedError' not in inspect.getsource(train_rnn.MultipleModels)
    assert inspect.signature(train_rnn.MultipleModels).parameters['rnnStateFeat'].default is None


def test_rnn_symbols_exported_and_bound():
    lib = C.CDLL(_lib._build.LIBPATH)
    for n in RNN_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _lib.EXPORTS, n


def test_envelope_queries():
    L = _lib.lib
    for dt in (_lib.F32, _lib.F64):
        assert L.gcrnn_rnn_supported(dt, 100, 5, 80, 1) == 1           # the k-step driver
        assert L.gcrnn_rnn_supported(dt, 100, 200, 59, 21) == 1        # the epicenter driver
        assert L.gcrnn_rnn_supported(dt, 256, 32, 1000, 64) == 1       # the large shape
        assert L.gcrnn_rnn_supported(dt, 4, 5, 80, 65) == 0            # one past the wave
        assert L.gcrnn_rnn_supported(dt, 0, 5, 80, 8) == 0
        assert L.gcrnn_rnn_supported(dt, 4, 5, 65537, 8) == 0
    assert L.gcrnn_rnn_supported(_lib.BF16, 4, 5, 80, 8) == 0
    assert ops.rnn_supported(torch.float32, 4, 5, 80, 64) and not ops.rnn_supported(torch.bfloat16, 4, 5, 80, 8)
    # the slot count is a function of the shape alone, at most 64, never 0 inside the envelope
    assert L.gcrnn_rnn_wgrad_slots(_lib.F32, 1, 1, 3, 1) == 1
    assert L.gcrnn_rnn_wgrad_slots(_lib.F32, 256, 32, 1000, 64) == 64
    assert L.gcrnn_rnn_wgrad_slots(_lib.F32, 100, 5, 80, 1) == L.gcrnn_rnn_wgrad_slots(_lib.F64, 100, 5, 80, 1) == 8
    assert L.gcrnn_rnn_wgrad_slots(_lib.F32, 4, 5, 80, 65) == 0


def test_entry_points_reject_bad_arguments_before_launch():
    L = _lib.lib
    p = C.c_void_p(64)                   # never dereferenced: every case below returns before a launch
    assert L.gcrnn_rnn_forward(_lib.F32, None, p, p, p, p, p, p, 2, 3, 4, 5, 0, None) == 3               # null x
    assert L.gcrnn_rnn_forward(_lib.F32, p, p, p, p, p, None, p, 2, 3, 4, 5, 0, None) == 3               # b_ih without b_hh
    assert L.gcrnn_rnn_forward(_lib.BF16, p, p, p, p, None, None, p, 2, 3, 4, 5, 0, None) == 1           # dtype
    assert L.gcrnn_rnn_forward(_lib.F32, p, p, p, p, None, None, p, 0, 3, 4, 5, 0, None) == 2            # B = 0
    assert L.gcrnn_rnn_forward(_lib.F32, p, p, p, p, None, None, p, 2, 3, 4, 5, 2, None) == 2            # act
    assert L.gcrnn_rnn_forward(_lib.F32, p, p, p, p, None, None, p, 2, 3, 4, 65, 0, None) == 4           # F_h > 64
    slots = L.gcrnn_rnn_wgrad_slots(_lib.F32, 2, 3, 4, 5)
    assert L.gcrnn_rnn_backward(_lib.F32, p, p, p, p, p, p, p, None, None, p, slots + 1, 2, 3, 4, 5, 0, None) == 6
    assert L.gcrnn_rnn_backward(_lib.F32, p, p, p, p, p, None, p, None, None, p, slots, 2, 3, 4, 5, 0, None) == 3
    assert L.gcrnn_rnn_backward(_lib.F64, p, p, p, p, p, p, p, None, None, p, slots, 2, 3, 4, 65, 1, None) == 4
