"""CPU: the GNN output heads keep the reference's surface -- the drivers' 'Sel' and 'GCRNNGNN' constructors, state_dict keys
and seeded initialisation bit for bit (G15 fixtures), the rejected branches, and the C ABI of the graph-filter layer kernel
(envelope and slot-capacity checks; no GPU compute is called)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import gated_gcrnns_amd.Utils.graphML as gml
import gated_gcrnns_amd.Modules.architectures as archit
from gated_gcrnns_amd import _lib

SYMBOLS = ['gcrnn_graph_filter_layer_supported', 'gcrnn_graph_filter_layer_forward', 'gcrnn_graph_filter_layer_backward',
           'gcrnn_graph_filter_layer_wgrad_slots']


@pytest.fixture(autouse=True)
def f64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)          # the drivers' setting
    yield
    torch.set_default_dtype(old)


def sel_quake(S):
    return archit.SelectionGNN([20, 21], [4], True, torch.nn.ReLU, [59], gml.NoPool, [1], [11], S)


def sel_kstep(S):
    return archit.SelectionGNN([1, 8, 1], [10, 10], True, torch.nn.ReLU, [50, 50], gml.NoPool, [1, 1], [], S)


def cls_gcrnngnn(S, tg):
    return archit.GatedGCRNNforClassification(1, 20, 4, 4, torch.tanh, torch.nn.ReLU, [11], S, True, tg, None,
                                              finalNonlinearity=torch.nn.ReLU, dimNodeSignals=[20, 1], nFilterTaps=[4],
                                              nSelectedNodes=[59], poolingFunction=gml.NoPool, poolingSize=[1])


def reg_gcrnngnn(S, tg, F, K):
    return archit.GatedGCRNNforRegression(1, 20, 2, 2, torch.tanh, torch.nn.ReLU, [], S, True, tg, None, 'oneMlp',
                                          torch.nn.ReLU, F, K, [50] * len(K), gml.NoPool, [1] * len(K))


CASES = [
    ('g15_sel_quake', lambda g: sel_quake(g['S'][0])),
    ('g15_sel_kstep', lambda g: sel_kstep(g['S'][0])),
    ('g15_cls_gcrnngnn_none', lambda g: cls_gcrnngnn(g['S'][0], False)),
    ('g15_cls_gcrnngnn_time', lambda g: cls_gcrnngnn(g['S'][0], True)),
    ('g15_reg_gcrnngnn_none', lambda g: reg_gcrnngnn(g['S'][0], False, [20, 1], [5])),
    ('g15_reg_gcrnngnn_time', lambda g: reg_gcrnngnn(g['S'][0], True, [20, 1], [5])),
    ('g15_reg_gcrnngnn_deep', lambda g: reg_gcrnngnn(g['S'][0], False, [20, 4, 1], [3, 2])),
]


@pytest.mark.parametrize('name,make', CASES, ids=[c[0] for c in CASES])
def test_state_dict_keys_and_seeded_init_match_reference(name, make):
    g = load_golden(name)
    torch.manual_seed(int(g['seed']))
    m = make(g)
    sd = m.state_dict()
    assert sorted(sd) == sorted(g['params'])
    for k in sd:
        assert np.array_equal(sd[k].numpy(), g['params'][k]), k
    m.load_state_dict({k: torch.tensor(v) for k, v in g['params'].items()})       # checkpoint compatible


def test_trace_model_init_matches_reference():
    g = load_golden('g15_trace_gcrnngnn')
    torch.manual_seed(157)
    m = cls_gcrnngnn(g['S'][0], False)
    for k, v in m.state_dict().items():
        assert np.array_equal(v.numpy(), g['params0'][k]), k


def test_selection_gnn_layout_mirrors_reference():
    S = np.eye(6) * 0.5
    m = archit.SelectionGNN([3, 4, 2], [2, 3], True, torch.nn.Tanh, [6, 6], gml.NoPool, [1, 1], [5, 1], S)
    assert len(m.GFL) == 6 and isinstance(m.GFL[0], gml.GraphFilter) and isinstance(m.GFL[1], torch.nn.Tanh)
    assert isinstance(m.GFL[2], gml.NoPool) and m.N == [6, 6, 6] and m.F == [3, 4, 2] and m.K == [2, 3]
    assert [type(l) for l in m.MLP] == [torch.nn.Linear, torch.nn.Tanh, torch.nn.Linear] and m.MLP[0].in_features == 12
    with pytest.raises(AssertionError):
        archit.SelectionGNN([3, 4], [2, 3], True, torch.nn.Tanh, [6, 6], gml.NoPool, [1, 1], [], S)


def test_nopool_mirrors_reference():
    p = gml.NoPool(5, 5, 1)
    p.addGSO(torch.eye(5))
    x = torch.randn(2, 3, 5)
    assert p(x) is x
    with pytest.raises(AssertionError):
        p(torch.randn(2, 3, 4))
    assert list(p.parameters()) == []


def test_aggregation_head_and_node_dropping_pooling_raise():
    S = np.eye(8) * 0.5
    with pytest.raises(NotImplementedError):            # AggregationGNN branch: no nSelectedNodes, pooling is not NoPool
        archit.GatedGCRNNforClassification(1, 4, 2, 2, torch.tanh, torch.nn.ReLU, [3], S, True, False, None,
                                           dimNodeSignals=[4, 1], nFilterTaps=[2], poolingFunction=gml.MaxPoolLocal)
    with pytest.raises(NotImplementedError):            # pooling that drops nodes
        archit.SelectionGNN([1, 2], [2], True, torch.nn.ReLU, [4], gml.NoPool, [1], [], S)
    with pytest.raises(NotImplementedError):
        archit.SelectionGNN([1, 2], [2], True, torch.nn.ReLU, [8], gml.MaxPoolLocal, [1], [], S)
    with pytest.raises(NotImplementedError):
        gml.MaxPoolLocal(8, 4, 1)


def test_kstep_driver_head_mismatch_fails_like_reference():
    """The k-step driver's GCRNNGNN head [5, 1] on F_h = 20 builds, and fails with the reference's AssertionError at forward
    (SelectionGNN.forward checks x.shape[1] == F[0] before anything runs)."""
    S = np.eye(10) * 0.5
    m = archit.GatedGCRNNforRegression(1, 20, 2, 2, torch.tanh, torch.nn.ReLU, [], S, True, False, None, 'oneMlp', None,
                                       [5, 1], [4], [10], gml.NoPool, [1])
    with pytest.raises(AssertionError):
        m.outputNN[0](torch.zeros(3, 20, 10))


def test_c_abi_symbols_are_exported_and_bound():
    for n in SYMBOLS:
        assert hasattr(_lib.lib, n) and n in _lib.EXPORTS


@pytest.mark.parametrize('dtype,N,nnz,Fin,Fout,K,uni', [
    (_lib.F64, 59, 400, 20, 21, 4, 0), (_lib.F32, 59, 400, 20, 21, 4, 0),        # epicenter 'Sel'
    (_lib.F64, 50, 1200, 1, 8, 10, 0), (_lib.F64, 50, 1200, 8, 1, 10, 0),         # k-step SelectionGNN
    (_lib.F64, 59, 400, 20, 1, 4, 0), (_lib.F64, 50, 1200, 20, 1, 5, 0),          # GCRNNGNN heads
    (_lib.BF16, 1000, 10000, 32, 1, 4, 0), (_lib.BF16, 1000, 10000, 64, 1, 5, 0),
    (_lib.BF16, 1000, 10000, 64, 1, 5, 1), (_lib.F32, 1000, 10000, 64, 1, 5, 0),  # the flagship head
    (_lib.BF16, 1000, 10000, 64, 4, 5, 0),
])
def test_supported_covers_the_driver_and_flagship_shapes(dtype, N, nnz, Fin, Fout, K, uni):
    assert _lib.lib.gcrnn_graph_filter_layer_supported(dtype, N, nnz, 1, Fin, Fout, K, uni) == 1
    assert 1 <= _lib.lib.gcrnn_graph_filter_layer_wgrad_slots(dtype, 8192, N, nnz, Fin, Fout, K, uni) <= 1024


def test_supported_rejects_outside_the_envelope():
    f = _lib.lib.gcrnn_graph_filter_layer_supported
    assert f(_lib.BF16, 1025, 10000, 1, 64, 1, 5, 0) == 0           # N > 1024
    assert f(_lib.BF16, 1000, 10000, 2, 64, 1, 5, 0) == 0           # E > 1
    assert f(_lib.F64, 1000, 100000, 1, 64, 64, 5, 0) == 0          # LDS image does not fit
    assert f(7, 100, 100, 1, 4, 1, 2, 0) == 0                       # dtype
    assert _lib.lib.gcrnn_graph_filter_layer_wgrad_slots(_lib.F32, 3, 100, 100, 4, 1, 2, 0) == 3


def test_backward_rejects_a_wrong_slot_capacity_before_launch():
    """Argument checks run on the host: fake (never dereferenced) pointers, GCRNN_ERR_WORKSPACE for a slot count other than
    gcrnn_graph_filter_layer_wgrad_slots, GCRNN_ERR_UNSUPPORTED / BAD_SHAPE / NULL_POINTER for the rest."""
    fake = 4096
    N, nnz, Fin, Fout, K, items = 100, 300, 8, 1, 3, 50
    slots = _lib.lib.gcrnn_graph_filter_layer_wgrad_slots(_lib.F32, items, N, nnz, Fin, Fout, K, 0)
    bwd = _lib.lib.gcrnn_graph_filter_layer_backward

    def call(slots_=slots, N_=N, E=1, x=fake, act=1):
        return bwd(_lib.F32, x, fake, fake, fake, fake, fake, fake, slots_, fake, fake, fake, 0.0, items, N_, nnz, E, Fin, Fout, K, act, None)
    assert call(slots_=slots + 1) == 6
    assert call(slots_=slots - 1) == 6
    assert call(N_=1025) == 4
    assert call(E=2) == 4
    assert call(x=None) == 3
    assert call(act=4) == 2
    fwd = _lib.lib.gcrnn_graph_filter_layer_forward
    assert fwd(_lib.F32, fake, fake, None, fake, fake, fake, fake, 0.0, items, 1025, nnz, 1, Fin, Fout, K, 0, None) == 4
