"""CPU: the host side of the small-graph per-node head entry points (gcrnn_small_dense_node_head_supported,
gcrnn_small_dense_forward_node_head, gcrnn_small_dense_backward_node_head) -- names in the header and the ctypes table, the query without a
device, and argument validation before any launch (dummy pointers: a call that got as far as a launch would fault, so a status code back is
the proof). No GPU compute is called."""
import ctypes as C
import os
import re

import torch

from conftest import ROOT
from gated_gcrnns_amd import _lib, ops

NEW = ('gcrnn_small_dense_node_head_supported', 'gcrnn_small_dense_forward_node_head', 'gcrnn_small_dense_backward_node_head')
OK, BAD_DTYPE, BAD_SHAPE, NULL, UNSUPPORTED = 0, 1, 2, 3, 4
F32, F64, BF16 = ops.dtype_code(torch.float32), ops.dtype_code(torch.float64), ops.dtype_code(torch.bfloat16)
ALL, LAST, NONE = 0, 1, 2              # GCRNN_SMALL_STATES_* of gcrnn.h


def _max_out():
    txt = open(os.path.join(ROOT, 'include', 'gcrnn.h')).read()
    return int(re.search(r'#define\s+GCRNN_SMALL_NODE_HEAD_MAX_OUT\s+(\d+)', txt).group(1))


def test_new_names_are_declared_and_bound():
    assert _max_out() == 8                                                         # node_linear_supported's bound on O
    txt = open(os.path.join(ROOT, 'include', 'gcrnn.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    declared = set(re.findall(r'\b(gcrnn_[a-z0-9_]+)\s*\(', txt))
    for n in NEW:
        assert n in declared, n
        assert n in _lib.EXPORTS, n
        assert hasattr(_lib.lib, n), n
    assert callable(ops.small_node_head_supported) and callable(ops.small_cell_regress)
    assert ops.node_linear_supported(20, _max_out(), torch.float64) and not ops.node_linear_supported(20, _max_out() + 1, torch.float64)


def test_query_answers_without_a_device(monkeypatch):
    monkeypatch.delenv('GCRNN_SMALL_GATHER', raising=False)
    lib = _lib.lib
    q = lib.gcrnn_small_dense_node_head_supported
    mx = _max_out()
    assert q(F64, 80, 1, 20, 5, 5, 1, 1, 1, 1) == 1                                # the k-step driver's shape, its training step with dX
    assert ops.small_node_head_supported(80, 1, 20, 5, 5, 1, torch.float64, True, True, dx=True)
    for code, dt in ((F32, torch.float32), (F64, torch.float64)):
        for backward in (0, 1):
            for gated in (0, 1):
                for dx in (0, 1):
                    for O in (1, 3, mx):
                        assert q(code, 59, 1, 20, 4, 4, O, backward, gated, dx) == 1, (code, O, backward, gated, dx)
                        assert ops.small_node_head_supported(59, 1, 20, 4, 4, O, dt, bool(backward), bool(gated), dx=bool(dx))
                    assert q(code, 59, 1, 20, 4, 4, 0, backward, gated, dx) == 0
                    assert q(code, 59, 1, 20, 4, 4, -1, backward, gated, dx) == 0
                    assert q(code, 59, 1, 20, 4, 4, mx + 1, backward, gated, dx) == 0
    for backward in (0, 1):
        assert q(BF16, 59, 1, 20, 4, 4, 1, backward, 0, 0) == 0
        assert q(F64, 300, 1, 20, 4, 4, 1, backward, 0, 0) == 0
    assert not ops.small_node_head_supported(59, 1, 20, 4, 4, 1, torch.bfloat16, False, False)
    # never more than the plain queries admit, over shapes on both sides of their edges
    for code in (F32, F64):
        for N, G, F, Ki, Ks in [(30, 2, 5, 3, 3), (88, 8, 20, 4, 4), (88, 8, 20, 5, 5), (120, 1, 20, 5, 5), (130, 1, 20, 2, 2), (200, 1, 8, 3, 3),
                                (300, 2, 8, 6, 6), (59, 1, 20, 9, 9), (257, 1, 4, 1, 1), (128, 1, 64, 5, 5)]:
            for backward in (0, 1):
                for gated in (0, 1):
                    plain = lib.gcrnn_small_dense_supported(code, N, G, F, Ki, Ks, backward, gated)
                    dxq = lib.gcrnn_small_dense_backward_dx_supported(code, N, G, F, Ki, Ks, gated)
                    for O in (1, mx):
                        got, got_dx = q(code, N, G, F, Ki, Ks, O, backward, gated, 0), q(code, N, G, F, Ki, Ks, O, backward, gated, 1)
                        assert got <= plain and got_dx <= (plain and dxq), (code, N, G, F, Ki, Ks, O)
                        if not plain:
                            assert got == 0 and got_dx == 0
                        if backward:                                               # the backward needs no LDS of its own for the head
                            assert got == plain and got_dx == (plain and dxq), (code, N, G, F, Ki, Ks, O)
    # the GPU tests' two-accumulator shape: fp32 only
    assert q(F32, 130, 1, 20, 2, 2, 1, 1, 1, 0) == 1 and q(F32, 130, 1, 20, 2, 2, 1, 0, 1, 0) == 1
    assert q(F64, 130, 1, 20, 2, 2, 1, 0, 0, 0) == 0
    monkeypatch.setenv('GCRNN_SMALL_GATHER', '1')              # the A/B switch to the gather family switches this path off too
    assert not ops.small_node_head_supported(59, 1, 20, 4, 4, 1, torch.float64, False, False)


def _fwd_args(dtype=F64, B=2, T=3, N=30, G=2, F=5, Kin=3, Kst=3, O=2, store=ALL, gs=(0, 0, 0), **ptr):
    one = C.c_void_p(16)
    names = ('X', 'h0', 'wA', 'wB', 'bias', 'gi', 'gf', 'Sdense', 'node_w', 'node_b', 'H', 'Y')
    p = {n: one for n in names}
    p['gi'] = p['gf'] = None
    p.update(ptr)
    return [dtype] + [p[n] for n in names] + [B, T, N, G, F, Kin, Kst, gs[0], gs[1], gs[2], O, store, None]


def test_forward_node_head_validates_before_launch():
    f = _lib.lib.gcrnn_small_dense_forward_node_head
    one = C.c_void_p(16)
    for n in ('X', 'h0', 'wA', 'wB', 'Sdense', 'node_w', 'Y', 'H'):
        assert f(*_fwd_args(**{n: None})) == NULL, n
    assert f(*_fwd_args(gi=one)) == NULL                                           # one gate without the other
    assert f(*_fwd_args(H=None, store=LAST)) == NULL
    assert f(*_fwd_args(Y=None, store=NONE)) == NULL
    assert f(*_fwd_args(X=None, dtype=BF16, N=0)) == NULL                          # the order: pointers, dtype, shape, support
    assert f(*_fwd_args(dtype=BF16)) == BAD_DTYPE
    assert f(*_fwd_args(dtype=9, N=0)) == BAD_DTYPE
    for kw in (dict(B=0), dict(T=-1), dict(N=0), dict(G=0), dict(F=-3), dict(Kin=0), dict(Kst=0), dict(O=0), dict(O=-2),
               dict(O=_max_out() + 1), dict(store=3), dict(store=-1)):
        assert f(*_fwd_args(**kw)) == BAD_SHAPE, kw
    assert f(*_fwd_args(N=300, O=0)) == BAD_SHAPE
    assert f(*_fwd_args(N=300)) == UNSUPPORTED
    assert f(*_fwd_args(dtype=F64, N=130, G=1, F=20, Kin=2, Kst=2)) == UNSUPPORTED   # fits in fp32 only
    assert f(*_fwd_args(H=None, store=NONE, N=300)) == UNSUPPORTED                   # (H may be NULL when no state is stored)
    assert f(*_fwd_args(node_b=None, N=300)) == UNSUPPORTED                          # (the head's bias is optional)


def _bwd_args(dtype=F64, B=2, T=3, N=30, G=2, F=5, Kin=3, Kst=3, O=2, **ptr):
    one = C.c_void_p(16)
    names = ('X', 'h0', 'H', 'dY', 'node_w', 'wA', 'wB', 'bias', 'gi', 'gf', 'Sdense', 'pA', 'pB', 'pb', 'dgi', 'dgf', 'dh0', 'dX')
    p = {n: one for n in names}
    p['gi'] = p['gf'] = p['dgi'] = p['dgf'] = None
    p.update(ptr)
    return [dtype] + [p[n] for n in names] + [B, T, N, G, F, Kin, Kst, 0, 0, 0, O, None]


def test_backward_node_head_validates_before_launch():
    f = _lib.lib.gcrnn_small_dense_backward_node_head
    one = C.c_void_p(16)
    for n in ('X', 'h0', 'H', 'dY', 'node_w', 'wA', 'wB', 'Sdense', 'pA', 'pB', 'pb'):
        assert f(*_bwd_args(**{n: None})) == NULL, n
    assert f(*_bwd_args(gf=one)) == NULL
    assert f(*_bwd_args(gi=one, gf=one)) == NULL                                   # gates without room for their gradients
    assert f(*_bwd_args(gi=one, gf=one, dgi=one)) == NULL
    assert f(*_bwd_args(dY=None, dtype=BF16, O=0)) == NULL
    assert f(*_bwd_args(dtype=BF16)) == BAD_DTYPE
    assert f(*_bwd_args(dtype=BF16, O=0)) == BAD_DTYPE
    for kw in (dict(B=0), dict(T=0), dict(N=-1), dict(G=0), dict(F=0), dict(Kin=0), dict(Kst=-2), dict(O=0), dict(O=_max_out() + 1)):
        assert f(*_bwd_args(**kw)) == BAD_SHAPE, kw
    assert f(*_bwd_args(N=300)) == UNSUPPORTED
    assert f(*_bwd_args(N=300, dX=None, dh0=None)) == UNSUPPORTED                  # (dX and dh0 are optional)
    # the dx image's LDS edge (test_small_input_grad_surface.py): with dX no, without it yes -- asked of the query, which the entry consults
    q = _lib.lib.gcrnn_small_dense_node_head_supported
    assert f(*_bwd_args(N=88, G=8, F=20, Kin=5, Kst=5)) == UNSUPPORTED
    assert q(F64, 88, 8, 20, 5, 5, 2, 1, 0, 1) == 0
    assert q(F64, 88, 8, 20, 5, 5, 2, 1, 0, 0) == 1


def test_regress_declines_on_the_host(monkeypatch):
    """GGCRNNCell.regress returns None (the model continues on the two-module path) for the off switch, a cell without a GSO and heads it
    does not take, before anything touches a device."""
    import gated_gcrnns_amd.Utils.graphML as gml
    cell = gml.GGCRNNCell(1, 4, 2, 2, torch.tanh, False, None, 1, True).double()
    X, h0 = torch.zeros(2, 3, 1, 6, dtype=torch.float64), torch.zeros(2, 4, 6, dtype=torch.float64)
    w = torch.zeros(1, 4, dtype=torch.float64)
    monkeypatch.setenv('GCRNN_NO_SMALL_NODE_HEAD', '1')
    assert cell.regress(X, h0, w, None) is None
    monkeypatch.delenv('GCRNN_NO_SMALL_NODE_HEAD')
    assert cell.regress(X, h0, w, None) is None                                    # no GSO stored
    cell.addGSO(torch.eye(6, dtype=torch.float64)[None])
    assert cell.regress(X, h0, torch.zeros(1, 5, dtype=torch.float64), None) is None           # not [O][F]
    assert cell.regress(X, h0, torch.zeros(9, 4, dtype=torch.float64), None) is None           # O above the maximum
    assert cell.regress(X, h0, w.float(), None) is None                                        # a head in another dtype
    assert callable(gml.GGCRNNCell._small_node_head_pays)
