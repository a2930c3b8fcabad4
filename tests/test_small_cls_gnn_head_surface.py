"""CPU: the host side of the classification model's Selection-GNN head on small graphs (gcrnn_small_dense_cls_gnn_head_supported,
gcrnn_small_dense_forward_cls_gnn_head, gcrnn_small_dense_backward_cls_gnn_head) -- names in the header and the ctypes table, the query
without a device over every shape the GPU tests use, argument validation before any launch (dummy pointers: a call that got as far as a
launch would fault, so a status code back is the proof), and the model's dispatch declining what is out of scope, shown by a spy on the
wrappers. No GPU compute is called."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT
from gated_gcrnns_amd import _lib, ops
import gated_gcrnns_amd.Utils.graphML as gml
import gated_gcrnns_amd.Modules.architectures as archit

NEW = ('gcrnn_small_dense_cls_gnn_head_supported', 'gcrnn_small_dense_forward_cls_gnn_head', 'gcrnn_small_dense_backward_cls_gnn_head')
OK, BAD_DTYPE, BAD_SHAPE, NULL, UNSUPPORTED = 0, 1, 2, 3, 4
F32, F64, BF16 = ops.dtype_code(torch.float32), ops.dtype_code(torch.float64), ops.dtype_code(torch.bfloat16)
ALL, LAST, NONE = 0, 1, 2              # GCRNN_SMALL_STATES_* of gcrnn.h
SWITCH = 'GCRNN_NO_SMALL_CLS_GNN_HEAD'

#          N, G,  F, Kin, Kst, K_o, C, T, B        (tests/test_small_cls_gnn_head.py's shapes)
SHAPES = {'quake59': (59, 1, 20, 4, 4, 4, 11, 3, 3),
          'exact16': (16, 2, 16, 2, 3, 2, 1, 2, 2),
          't1n17': (17, 1, 5, 3, 2, 5, 3, 1, 1),
          'k1n17': (17, 1, 5, 2, 2, 1, 19, 2, 1),
          'five80': (80, 1, 20, 5, 5, 5, 5, 4, 2),
          'two130': (130, 1, 20, 2, 2, 2, 2, 2, 2)}       # fp32 only


def _define(name):
    txt = open(os.path.join(ROOT, 'include', 'gcrnn.h')).read()
    return int(re.search(r'#define\s+%s\s+(\d+)' % name, txt).group(1))


def test_new_names_are_declared_and_bound():
    txt = open(os.path.join(ROOT, 'include', 'gcrnn.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    declared = set(re.findall(r'\b(gcrnn_[a-z0-9_]+)\s*\(', txt))
    for n in NEW:
        assert n in declared, n
        assert n in _lib.EXPORTS, n
        assert hasattr(_lib.lib, n), n
    assert callable(ops.small_cls_gnn_head_supported) and callable(ops.small_cell_classify_gnn)
    assert callable(gml.GGCRNNCell.classify_gnn) and callable(gml.GGCRNNCell._small_cls_gnn_head_pays)
    assert _define('GCRNN_SMALL_NODE_HEAD_MAX_OUT') == 8 and _define('GCRNN_SMALL_HEAD_MAX_CLASSES') == 1024


def test_query_answers_without_a_device(monkeypatch):
    monkeypatch.delenv('GCRNN_SMALL_GATHER', raising=False)
    q = _lib.lib.gcrnn_small_dense_cls_gnn_head_supported
    for name, (N, G, F, Kin, Kst, Ko, Cl, T, B) in SHAPES.items():
        for code, dt in ((F32, torch.float32), (F64, torch.float64)):
            if name == 'two130' and dt == torch.float64:
                for backward in (0, 1):
                    assert q(code, N, G, F, Kin, Kst, Ko, Cl, backward, 0, 0) == 0     # fits in fp32 only, as the cell itself
                continue
            for backward in (0, 1):
                for gated in (0, 1):
                    for dx in (0, 1):
                        assert q(code, N, G, F, Kin, Kst, Ko, Cl, backward, gated, dx) == 1, (name, code, backward, gated, dx)
                        assert ops.small_cls_gnn_head_supported(N, G, F, Kin, Kst, Ko, Cl, dt, bool(backward), bool(gated), dx=bool(dx)), name
    # the model tests' cell (N = 59, K = 4, C = 11) with heads on both sides of K
    for Ko in range(1, 9):
        assert q(F64, 59, 1, 20, 4, 4, Ko, 11, 1, 1, 1) == 1 and q(F32, 59, 1, 20, 4, 4, Ko, 11, 0, 1, 0) == 1
    for code in (F32, F64):
        for backward in (0, 1):
            for Ko in (0, 9, -1):
                assert q(code, 59, 1, 20, 4, 4, Ko, 11, backward, 0, 0) == 0, Ko
            for Cl in (0, 1025, -1):
                assert q(code, 59, 1, 20, 4, 4, 4, Cl, backward, 0, 0) == 0, Cl
            assert q(code, 59, 1, 20, 4, 4, 8, 1024, backward, 0, 0) == 1
            assert q(code, 300, 1, 20, 4, 4, 2, 3, backward, 0, 0) == 0
    for backward in (0, 1):
        assert q(BF16, 59, 1, 20, 4, 4, 4, 11, backward, 0, 0) == 0
    assert not ops.small_cls_gnn_head_supported(59, 1, 20, 4, 4, 4, 11, torch.bfloat16, False, False)
    assert not ops.small_cls_gnn_head_supported(59, 1, 20, 4, 4, 0, 11, torch.float64, False, False)
    assert not ops.small_cls_gnn_head_supported(59, 1, 20, 4, 4, 9, 11, torch.float64, False, False)
    assert not ops.small_cls_gnn_head_supported(59, 1, 20, 4, 4, 4, 0, torch.float64, False, False)
    assert not ops.small_cls_gnn_head_supported(59, 1, 20, 4, 4, 4, 1025, torch.float64, True, False)
    assert ops.small_cls_gnn_head_supported(59, 1, 20, 4, 4, 4, 11, torch.float64, True, True, dx=True, E=1)
    assert not ops.small_cls_gnn_head_supported(59, 1, 20, 4, 4, 4, 11, torch.float64, False, False, E=2)       # E != 1: at the Python level
    # never more than the cell's own queries admit; the forward never more than the every-state graph-filter head (it adds the vector v)
    lib = _lib.lib
    for code in (F32, F64):
        for N, G, F, Ki, Ks in [(30, 2, 5, 3, 3), (88, 8, 20, 4, 4), (88, 8, 20, 5, 5), (120, 1, 20, 5, 5), (130, 1, 20, 2, 2), (200, 1, 8, 3, 3),
                                (300, 2, 8, 6, 6), (59, 1, 20, 9, 9), (257, 1, 4, 1, 1), (128, 1, 64, 5, 5)]:
            for backward in (0, 1):
                for gated in (0, 1):
                    for dx in (0, 1):
                        for Ko in (1, 5, 8):
                            got = q(code, N, G, F, Ki, Ks, Ko, 11, backward, gated, dx)
                            assert got <= lib.gcrnn_small_dense_supported(code, N, G, F, Ki, Ks, backward, gated)
                            if dx:
                                assert got <= lib.gcrnn_small_dense_backward_dx_supported(code, N, G, F, Ki, Ks, gated)
                            if not backward:
                                assert got <= lib.gcrnn_small_dense_gnn_head_supported(code, N, G, F, Ki, Ks, Ko, 0, gated, 0)
    monkeypatch.setenv('GCRNN_SMALL_GATHER', '1')              # the A/B switch to the gather family switches this path off too
    assert not ops.small_cls_gnn_head_supported(59, 1, 20, 4, 4, 4, 11, torch.float64, False, False)


def _fwd_args(dtype=F64, B=2, T=3, N=30, G=2, F=5, Kin=3, Kst=3, Ko=2, Cl=4, act=1, store=ALL, **ptr):
    one = C.c_void_p(16)
    names = ('X', 'h0', 'wA', 'wB', 'bias', 'gi', 'gf', 'Sdense', 'head_w', 'head_b', 'lin_w', 'lin_b', 'H', 'V', 'logits')
    p = {n: one for n in names}
    p['gi'] = p['gf'] = None
    p.update(ptr)
    return [dtype] + [p[n] for n in names] + [B, T, N, G, F, Kin, Kst, 0, 0, 0, Ko, Cl, act, store, None]


SHAPE_ERRORS = (dict(B=0), dict(T=-1), dict(N=0), dict(G=0), dict(F=-3), dict(Kin=0), dict(Kst=0), dict(Ko=0), dict(Ko=-2), dict(Ko=9),
                dict(Cl=0), dict(Cl=1025), dict(act=4), dict(act=-1))


def test_forward_validates_before_launch():
    f = _lib.lib.gcrnn_small_dense_forward_cls_gnn_head
    one = C.c_void_p(16)
    for n in ('X', 'h0', 'wA', 'wB', 'Sdense', 'head_w', 'lin_w', 'logits', 'H'):
        assert f(*_fwd_args(**{n: None})) == NULL, n
    assert f(*_fwd_args(gi=one)) == NULL                                           # one gate without the other
    assert f(*_fwd_args(H=None, store=LAST)) == NULL
    assert f(*_fwd_args(X=None, dtype=BF16, N=0)) == NULL                          # the order: pointers, dtype, shape, support
    assert f(*_fwd_args(dtype=BF16, N=0)) == BAD_DTYPE
    assert f(*_fwd_args(dtype=BF16)) == BAD_DTYPE
    for kw in SHAPE_ERRORS + (dict(store=3), dict(store=-1)):
        assert f(*_fwd_args(**kw)) == BAD_SHAPE, kw
        assert f(*_fwd_args(**dict(dict(N=300), **kw))) == BAD_SHAPE, kw                         # the shape before the support query
    assert f(*_fwd_args(N=300)) == UNSUPPORTED
    assert f(*_fwd_args(dtype=F64, N=130, G=1, F=20, Kin=2, Kst=2)) == UNSUPPORTED   # fits in fp32 only
    assert f(*_fwd_args(H=None, store=NONE, N=300)) == UNSUPPORTED                   # (H may be NULL when no state is stored)
    assert f(*_fwd_args(head_b=None, lin_b=None, V=None, N=300)) == UNSUPPORTED      # (both biases and V are optional)


def _bwd_args(dtype=F64, B=2, T=3, N=30, G=2, F=5, Kin=3, Kst=3, Ko=2, Cl=4, act=1, **ptr):
    one = C.c_void_p(16)
    names = ('X', 'h0', 'H', 'dlogits', 'lin_w', 'V', 'head_w', 'wA', 'wB', 'bias', 'gi', 'gf', 'Sdense', 'pA', 'pB', 'pb', 'dgi', 'dgf',
             'dh0', 'dX', 'dU')
    p = {n: one for n in names}
    p['gi'] = p['gf'] = p['dgi'] = p['dgf'] = None
    p.update(ptr)
    return [dtype] + [p[n] for n in names] + [B, T, N, G, F, Kin, Kst, 0, 0, 0, Ko, Cl, act, None]


def test_backward_validates_before_launch():
    f = _lib.lib.gcrnn_small_dense_backward_cls_gnn_head
    one = C.c_void_p(16)
    for n in ('X', 'h0', 'H', 'dlogits', 'lin_w', 'V', 'head_w', 'wA', 'wB', 'Sdense', 'pA', 'pB', 'pb', 'dU'):
        assert f(*_bwd_args(**{n: None})) == NULL, n
    assert f(*_bwd_args(gi=one)) == NULL                                           # one gate without the other
    assert f(*_bwd_args(gi=one, gf=one)) == NULL                                   # gates without room for their gradients
    assert f(*_bwd_args(gi=one, gf=one, dgi=one)) == NULL
    assert f(*_bwd_args(dU=None, dtype=BF16, N=0)) == NULL                         # the order: pointers, dtype, shape, support
    assert f(*_bwd_args(dtype=BF16, N=0)) == BAD_DTYPE
    for kw in SHAPE_ERRORS:
        assert f(*_bwd_args(**kw)) == BAD_SHAPE, kw
        assert f(*_bwd_args(**dict(dict(N=300), **kw))) == BAD_SHAPE, kw
    assert f(*_bwd_args(N=300)) == UNSUPPORTED
    assert f(*_bwd_args(N=300, dX=None, dh0=None, bias=None)) == UNSUPPORTED       # (dX, dh0 and the bias are optional)
    assert f(*_bwd_args(dtype=F64, N=130, G=1, F=20, Kin=2, Kst=2)) == UNSUPPORTED   # fits in fp32 only
    assert f(*_bwd_args(gi=one, gf=one, dgi=one, dgf=one, N=300)) == UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------- the model's dispatch
class _Declined(Exception):
    pass


@pytest.fixture
def spy(monkeypatch):
    """Counts GGCRNNCell.classify_gnn's calls and answers; ops.small_cell_classify_gnn -- the only way onto the new kernels -- raises, and
    the cell's own forward is cut short, so nothing here reaches a device."""
    calls = dict(asked=0, declined=0)
    real = gml.GGCRNNCell.classify_gnn

    def classify_gnn(self, *a, **kw):
        calls['asked'] += 1
        out = real(self, *a, **kw)
        assert out is None
        calls['declined'] += 1
        return out

    def taken(*a, **kw):
        raise AssertionError('the new path was taken')

    def old_path(self, X, h0, last_only=False):
        raise _Declined()
    monkeypatch.setattr(gml.GGCRNNCell, 'classify_gnn', classify_gnn)
    monkeypatch.setattr(ops, 'small_cell_classify_gnn', taken)
    monkeypatch.setattr(gml.GGCRNNCell, 'forward', old_path)
    monkeypatch.delenv(SWITCH, raising=False)
    monkeypatch.delenv('GCRNN_SMALL_CLS_GNN_HEAD', raising=False)
    monkeypatch.delenv('GCRNN_SMALL_GATHER', raising=False)
    return calls


def _cls(F_o, K_o, mlp=(3,), spatial=None, N=12, sigma2=torch.nn.ReLU):
    torch.manual_seed(3)
    S = torch.rand(1, N, N, dtype=torch.float64) / N
    return archit.GatedGCRNNforClassification(1, 4, 2, 2, torch.tanh, sigma2, list(mlp), S, True, False, spatial, None,
                                              list(F_o), list(K_o), [N] * len(K_o), gml.NoPool, [1] * len(K_o)).double()


def _run(m, dt=torch.float64):
    N = m.N
    with pytest.raises(_Declined):
        m(torch.zeros(2, 3, 1, N, dtype=dt), torch.zeros(2, 4, N, dtype=dt))


def test_model_declines_what_is_out_of_scope(spy, monkeypatch):
    _run(_cls([4, 3, 1], [2, 2]))                              # a two-layer head
    assert spy == dict(asked=0, declined=0)                    # (declined by the model before the cell is asked)
    _run(_cls([4, 2], [3]))                                    # F_out = 2
    assert spy == dict(asked=0, declined=0)
    _run(_cls([4, 1], [3], mlp=(5, 3)))                        # an MLP of two layers
    assert spy == dict(asked=0, declined=0)
    _run(_cls([4, 1], [3], mlp=()))                            # no MLP at all
    assert spy == dict(asked=0, declined=0)
    _run(_cls([4, 1], [3], sigma2=torch.nn.LeakyReLU))         # the Linear sits behind the activation inside the launch: fused ones only
    assert spy == dict(asked=0, declined=0)
    half = _cls([4, 1], [3])
    half.stateGCRNN.float()                                    # head parameters in another dtype than the states
    _run(half, torch.float32)
    assert spy == dict(asked=0, declined=0)
    half = _cls([4, 1], [3])
    half.outputNN[0].MLP.float()                               # the Linear alone in another dtype: the cell is asked and declines
    _run(half)
    assert spy == dict(asked=1, declined=1)
    _run(_cls([4, 1], [9]))                                    # K_o above the maximum
    assert spy == dict(asked=2, declined=2)
    _run(_cls([4, 1], [3], spatial='edge'))                    # edge gating
    assert spy == dict(asked=3, declined=3)
    monkeypatch.setenv(SWITCH, '1')                            # the off switch, read at every call
    _run(_cls([4, 1], [3]))
    assert spy == dict(asked=4, declined=4)
    monkeypatch.delenv(SWITCH)
    m = _cls([4, 1], [3])                                      # in scope: the route accepts, and stops at the tensors not being on a device
    with pytest.raises(ops.GcrnnError, match='no CPU path'):
        m(torch.zeros(2, 3, 1, m.N, dtype=torch.float64), torch.zeros(2, 4, m.N, dtype=torch.float64))
    assert spy == dict(asked=5, declined=4)


def test_classify_gnn_declines_on_the_host(monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)
    cell = gml.GGCRNNCell(1, 4, 2, 2, torch.tanh, False, None, 1, True).double()
    X, h0 = torch.zeros(2, 3, 1, 6, dtype=torch.float64), torch.zeros(2, 4, 6, dtype=torch.float64)
    w, lw = torch.zeros(1, 1, 3, 4, dtype=torch.float64), torch.zeros(5, 6, dtype=torch.float64)
    assert cell.classify_gnn(X, h0, w, None, 'relu', lw, None) is None                      # no GSO stored
    cell.addGSO(torch.eye(6, dtype=torch.float64)[None])
    monkeypatch.setenv(SWITCH, '1')
    assert cell.classify_gnn(X, h0, w, None, 'relu', lw, None) is None
    monkeypatch.delenv(SWITCH)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    assert cell.classify_gnn(X, h0, z(2, 1, 3, 4), None, 'relu', lw, None) is None          # F_out = 2
    assert cell.classify_gnn(X, h0, z(1, 2, 3, 4), None, 'relu', lw, None) is None          # E = 2
    assert cell.classify_gnn(X, h0, z(1, 1, 9, 4), None, 'relu', lw, None) is None          # K_o above the maximum
    assert cell.classify_gnn(X, h0, z(1, 1, 3, 5), None, 'relu', lw, None) is None          # not [K_o][F]
    assert cell.classify_gnn(X, h0, w.float(), None, 'relu', lw, None) is None              # a filter in another dtype
    assert cell.classify_gnn(X, h0, w, None, 'softplus', lw, None) is None                  # not one of the layer's codes
    assert cell.classify_gnn(X, h0, w, None, 'relu', z(5, 7), None) is None                 # not [C][N]
    assert cell.classify_gnn(X, h0, w, None, 'relu', z(5, 6, 1), None) is None
    assert cell.classify_gnn(X, h0, w, None, 'relu', lw.float(), None) is None              # a read-out in another dtype
    assert cell.classify_gnn(X, h0, w, None, 'relu', lw, z(5).float()) is None
    assert cell.classify_gnn(X, h0, w, None, 'relu', z(1025, 6), None) is None              # more classes than the kernel takes
