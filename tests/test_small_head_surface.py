"""CPU: the host side of the small-graph read-out entry points (gcrnn_small_dense_head_supported, gcrnn_small_dense_forward_head,
gcrnn_small_dense_backward_head) -- names in the header and the ctypes table, the query without a device, and argument validation before
any launch (dummy pointers: a call that got as far as a launch would fault, so a status code back is the proof). No GPU compute is called."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT
from gated_gcrnns_amd import _lib, ops

NEW = ('gcrnn_small_dense_head_supported', 'gcrnn_small_dense_forward_head', 'gcrnn_small_dense_backward_head')
OK, BAD_DTYPE, BAD_SHAPE, NULL, UNSUPPORTED = 0, 1, 2, 3, 4
F32, F64, BF16 = ops.dtype_code(torch.float32), ops.dtype_code(torch.float64), ops.dtype_code(torch.bfloat16)
ALL, LAST, NONE = 0, 1, 2              # GCRNN_SMALL_STATES_* of gcrnn.h


def test_new_names_are_declared_and_bound():
    txt = open(os.path.join(ROOT, 'include', 'gcrnn.h')).read()
    max_classes = int(re.search(r'#define\s+GCRNN_SMALL_HEAD_MAX_CLASSES\s+(\d+)', txt).group(1))
    assert max_classes >= 64
    assert re.search(r'GCRNN_SMALL_STATES_ALL = 0, GCRNN_SMALL_STATES_LAST = 1, GCRNN_SMALL_STATES_NONE = 2', txt)
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    declared = set(re.findall(r'\b(gcrnn_[a-z0-9_]+)\s*\(', txt))
    for n in NEW:
        assert n in declared, n
        assert n in _lib.EXPORTS, n
        assert hasattr(_lib.lib, n), n
    assert callable(ops.small_head_supported) and callable(ops.small_cell_classify)
    assert (ops.SMALL_STATES_ALL, ops.SMALL_STATES_LAST, ops.SMALL_STATES_NONE) == (ALL, LAST, NONE)
    lib = _lib.lib
    assert lib.gcrnn_small_dense_head_supported(F64, 59, 1, 20, 4, 4, max_classes, 1, 1, 1) == 1
    assert lib.gcrnn_small_dense_head_supported(F64, 59, 1, 20, 4, 4, max_classes + 1, 0, 0, 0) == 0


def test_query_answers_without_a_device(monkeypatch):
    monkeypatch.delenv('GCRNN_SMALL_GATHER', raising=False)
    lib = _lib.lib
    for code, dt in ((F32, torch.float32), (F64, torch.float64)):
        for backward in (0, 1):
            for gated in (0, 1):
                for dx in (0, 1):
                    assert lib.gcrnn_small_dense_head_supported(code, 59, 1, 20, 4, 4, 11, backward, gated, dx) == 1, (code, backward, gated, dx)
                    assert ops.small_head_supported(59, 1, 20, 4, 4, 11, dt, bool(backward), bool(gated), dx=bool(dx))
    for backward in (0, 1):
        assert lib.gcrnn_small_dense_head_supported(BF16, 59, 1, 20, 4, 4, 11, backward, 0, 0) == 0
        assert lib.gcrnn_small_dense_head_supported(F64, 300, 1, 20, 4, 4, 11, backward, 0, 0) == 0
        assert lib.gcrnn_small_dense_head_supported(F64, 59, 1, 20, 4, 4, 0, backward, 0, 0) == 0
        assert lib.gcrnn_small_dense_head_supported(F64, 59, 1, 20, 4, 4, 64, backward, 1, 0) == 1
    assert not ops.small_head_supported(59, 1, 20, 4, 4, 11, torch.bfloat16, False, False)
    # never more than the plain queries admit, over shapes on both sides of their edges
    for code in (F32, F64):
        for N, G, F, Ki, Ks in [(30, 2, 5, 3, 3), (88, 8, 20, 4, 4), (88, 8, 20, 5, 5), (120, 1, 20, 5, 5), (130, 1, 20, 2, 2), (200, 1, 8, 3, 3),
                                (300, 2, 8, 6, 6), (59, 1, 20, 9, 9), (257, 1, 4, 1, 1), (128, 1, 64, 5, 5)]:
            for backward in (0, 1):
                for gated in (0, 1):
                    plain = lib.gcrnn_small_dense_supported(code, N, G, F, Ki, Ks, backward, gated)
                    assert lib.gcrnn_small_dense_head_supported(code, N, G, F, Ki, Ks, 11, backward, gated, 0) == plain, (code, N, G, F, Ki, Ks)
                    dxq = lib.gcrnn_small_dense_backward_dx_supported(code, N, G, F, Ki, Ks, gated)
                    assert lib.gcrnn_small_dense_head_supported(code, N, G, F, Ki, Ks, 11, backward, gated, 1) == (plain and dxq), (code, N, G, F, Ki, Ks)
    # the GPU tests' two-accumulator shape: fp32 only
    assert lib.gcrnn_small_dense_head_supported(F32, 130, 1, 20, 2, 2, 11, 1, 1, 0) == 1
    assert lib.gcrnn_small_dense_head_supported(F64, 130, 1, 20, 2, 2, 11, 0, 0, 0) == 0
    monkeypatch.setenv('GCRNN_SMALL_GATHER', '1')              # the A/B switch to the gather family switches the read-out path off too
    assert not ops.small_head_supported(59, 1, 20, 4, 4, 11, torch.float64, False, False)


def _fwd_args(dtype=F64, B=2, T=3, N=30, G=2, F=5, Kin=3, Kst=3, C_=4, store=ALL, gs=(0, 0, 0), **ptr):
    one = C.c_void_p(16)
    names = ('X', 'h0', 'wA', 'wB', 'bias', 'gi', 'gf', 'Sdense', 'head_w', 'head_b', 'H', 'logits')
    p = {n: one for n in names}
    p['gi'] = p['gf'] = None
    p.update(ptr)
    return [dtype] + [p[n] for n in names] + [B, T, N, G, F, Kin, Kst, gs[0], gs[1], gs[2], C_, store, None]


def test_forward_head_validates_before_launch():
    f = _lib.lib.gcrnn_small_dense_forward_head
    one = C.c_void_p(16)
    for n in ('X', 'h0', 'wA', 'wB', 'Sdense', 'logits', 'H'):
        assert f(*_fwd_args(**{n: None})) == NULL, n
    assert f(*_fwd_args(gi=one)) == NULL                                           # one gate without the other
    assert f(*_fwd_args(head_w=None)) == NULL                                      # logits without a read-out
    assert f(*_fwd_args(head_w=None, logits=None, C_=0)) == NULL                   # a bias without a read-out
    assert f(*_fwd_args(head_w=None, head_b=None, logits=None, C_=0, store=NONE)) == NULL      # nothing left to write
    assert f(*_fwd_args(H=None, store=LAST)) == NULL
    assert f(*_fwd_args(dtype=BF16)) == BAD_DTYPE
    assert f(*_fwd_args(dtype=9)) == BAD_DTYPE
    for kw in (dict(B=0), dict(T=-1), dict(N=0), dict(G=0), dict(F=-3), dict(Kin=0), dict(Kst=0), dict(C_=0), dict(store=3), dict(store=-1)):
        assert f(*_fwd_args(**kw)) == BAD_SHAPE, kw
    assert f(*_fwd_args(head_w=None, head_b=None, logits=None, C_=2, store=LAST)) == BAD_SHAPE         # classes without a read-out
    assert f(*_fwd_args(N=300)) == UNSUPPORTED
    assert f(*_fwd_args(N=300, head_w=None, head_b=None, logits=None, C_=0, store=LAST)) == UNSUPPORTED
    assert f(*_fwd_args(C_=100000)) == UNSUPPORTED
    assert f(*_fwd_args(dtype=F64, N=130, G=1, F=20, Kin=2, Kst=2)) == UNSUPPORTED   # fits in fp32 only
    assert f(*_fwd_args(H=None, store=NONE, N=300)) == UNSUPPORTED                   # (H may be NULL when no state is stored)


def _bwd_args(dtype=F64, B=2, T=3, N=30, G=2, F=5, Kin=3, Kst=3, C_=4, **ptr):
    one = C.c_void_p(16)
    names = ('X', 'h0', 'H', 'dlogits', 'head_w', 'wA', 'wB', 'bias', 'gi', 'gf', 'Sdense', 'pA', 'pB', 'pb', 'dgi', 'dgf', 'dh0', 'dX')
    p = {n: one for n in names}
    p['gi'] = p['gf'] = p['dgi'] = p['dgf'] = None
    p.update(ptr)
    return [dtype] + [p[n] for n in names] + [B, T, N, G, F, Kin, Kst, 0, 0, 0, C_, None]


def test_backward_head_validates_before_launch():
    f = _lib.lib.gcrnn_small_dense_backward_head
    one = C.c_void_p(16)
    for n in ('X', 'h0', 'H', 'dlogits', 'head_w', 'wA', 'wB', 'Sdense', 'pA', 'pB', 'pb'):
        assert f(*_bwd_args(**{n: None})) == NULL, n
    assert f(*_bwd_args(gf=one)) == NULL
    assert f(*_bwd_args(gi=one, gf=one)) == NULL                                   # gates without room for their gradients
    assert f(*_bwd_args(gi=one, gf=one, dgi=one)) == NULL
    assert f(*_bwd_args(dtype=BF16)) == BAD_DTYPE
    for kw in (dict(B=0), dict(T=0), dict(N=-1), dict(G=0), dict(F=0), dict(Kin=0), dict(Kst=-2), dict(C_=0)):
        assert f(*_bwd_args(**kw)) == BAD_SHAPE, kw
    assert f(*_bwd_args(N=300)) == UNSUPPORTED
    assert f(*_bwd_args(N=300, dX=None, dh0=None)) == UNSUPPORTED
    assert f(*_bwd_args(C_=100000)) == UNSUPPORTED
    # the dx image's LDS edge (test_small_input_grad_surface.py): with dX no, without it yes -- asked of the query, which the entry consults
    lib = _lib.lib
    assert f(*_bwd_args(N=88, G=8, F=20, Kin=5, Kst=5)) == UNSUPPORTED
    assert lib.gcrnn_small_dense_head_supported(F64, 88, 8, 20, 5, 5, 4, 1, 0, 1) == 0
    assert lib.gcrnn_small_dense_head_supported(F64, 88, 8, 20, 5, 5, 4, 1, 0, 0) == 1


def test_classify_declines_on_the_host(monkeypatch):
    """GGCRNNCell.classify returns None (the model continues on the two-module path) for the off switch and for a cell without a GSO,
    before anything touches a device."""
    import gated_gcrnns_amd.Utils.graphML as gml
    cell = gml.GGCRNNCell(1, 4, 2, 2, torch.tanh, False, None, 1, True).double()
    X, h0 = torch.zeros(2, 3, 1, 6, dtype=torch.float64), torch.zeros(2, 4, 6, dtype=torch.float64)
    w = torch.zeros(3, 24, dtype=torch.float64)
    monkeypatch.setenv('GCRNN_NO_SMALL_HEAD', '1')
    assert cell.classify(X, h0, w, None) is None
    monkeypatch.delenv('GCRNN_NO_SMALL_HEAD')
    assert cell.classify(X, h0, w, None) is None                                   # no GSO stored
    # fp32 inference beyond T = 20 keeps the all-states launch (measured slower there); fp64 and short fp32 sequences do not
    pays = gml.GGCRNNCell._small_last_state_pays
    assert pays(torch.zeros(1, 200, 1, 6, dtype=torch.float64)) and pays(torch.zeros(1, 20, 1, 6)) and not pays(torch.zeros(1, 21, 1, 6))
