"""CPU: the host side of the small-graph input-gradient entry points -- names in the header and the ctypes table, argument validation
before any launch, and the dx predicate (ops.small_input_grad_supported against the C queries, the shapes the GPU tests rely on and the
shapes that must stay on the composed path). No GPU compute is called."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT
from gated_gcrnns_amd import _lib, ops

NEW = ('gcrnn_small_backward_dx', 'gcrnn_small_dense_backward_dx', 'gcrnn_small_dense_backward_dx_supported',
       'gcrnn_small_gates_backward_dx')
OK, BAD_DTYPE, BAD_SHAPE, NULL, UNSUPPORTED = 0, 1, 2, 3, 4
F32, F64 = ops.dtype_code(torch.float32), ops.dtype_code(torch.float64)


def test_new_names_are_declared_and_bound():
    txt = open(os.path.join(ROOT, 'include', 'gcrnn.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    declared = set(re.findall(r'\b(gcrnn_[a-z0-9_]+)\s*\(', txt))
    for n in NEW:
        assert n in declared, n
        assert n in _lib.EXPORTS, n
        assert hasattr(_lib.lib, n), n
    assert callable(ops.small_input_grad_supported)


def _gather_args(dX, dtype=F64, B=2, T=3, N=30, G=2, F=5, Kin=3, Kst=3, nnz=90, X=16):
    one = C.c_void_p(16)
    p = [C.c_void_p(X) if X else None] + [one] * 20           # X .. dgf, dh0
    return [dtype] + p + [dX, B, T, N, G, F, Kin, Kst, nnz, None]


def test_gather_dx_entry_validates_before_launch():
    lib = _lib.lib
    one = C.c_void_p(16)
    assert lib.gcrnn_small_backward_dx(*_gather_args(None)) == NULL
    assert lib.gcrnn_small_backward_dx(*_gather_args(one, X=0)) == NULL
    assert lib.gcrnn_small_backward_dx(*_gather_args(one, dtype=7)) == BAD_DTYPE
    for kw in (dict(B=0), dict(T=0), dict(N=0), dict(G=-1), dict(F=0), dict(Kin=0), dict(Kst=-2), dict(nnz=-1)):
        assert lib.gcrnn_small_backward_dx(*_gather_args(one, **kw)) == BAD_SHAPE, kw
    assert lib.gcrnn_small_backward_dx(*_gather_args(one, Kin=6, Kst=6)) == UNSUPPORTED        # K <= 5 on the gather family
    assert lib.gcrnn_small_backward_dx(*_gather_args(one, N=1030, nnz=4000)) == UNSUPPORTED


def _dense_args(dX, dtype=F64, B=2, T=3, N=30, G=2, F=5, Kin=3, Kst=3, X=16):
    one = C.c_void_p(16)
    p = [C.c_void_p(X) if X else None] + [one] * 15           # X .. dh0
    return [dtype] + p + [dX, B, T, N, G, F, Kin, Kst, 0, 0, 0, None]


def test_dense_dx_entry_validates_before_launch():
    lib = _lib.lib
    one = C.c_void_p(16)
    assert lib.gcrnn_small_dense_backward_dx(*_dense_args(None)) == NULL
    assert lib.gcrnn_small_dense_backward_dx(*_dense_args(one, X=0)) == NULL
    assert lib.gcrnn_small_dense_backward_dx(*_dense_args(one, dtype=9)) == BAD_DTYPE
    for kw in (dict(B=0), dict(T=-1), dict(N=0), dict(G=0), dict(F=-3), dict(Kin=0), dict(Kst=0)):
        assert lib.gcrnn_small_dense_backward_dx(*_dense_args(one, **kw)) == BAD_SHAPE, kw
    assert lib.gcrnn_small_dense_backward_dx(*_dense_args(one, N=300)) == UNSUPPORTED
    assert lib.gcrnn_small_dense_backward_dx(*_dense_args(one, N=88, G=8, F=20, Kin=5, Kst=5)) == UNSUPPORTED       # the dx image's LDS edge


def _gates_args(pdX, dtype=F64, B=2, T=3, N=30, G=2, F=5, Kin=3, Kst=3, X=16):
    one = C.c_void_p(16)
    p = [C.c_void_p(X) if X else None] + [one] * 13           # X .. pdh0
    return [dtype] + p + [pdX, B, T, N, G, F, Kin, Kst, None]


def test_gates_dx_entry_validates_before_launch():
    lib = _lib.lib
    one = C.c_void_p(16)
    assert lib.gcrnn_small_gates_backward_dx(*_gates_args(None)) == NULL
    assert lib.gcrnn_small_gates_backward_dx(*_gates_args(one, X=0)) == NULL
    assert lib.gcrnn_small_gates_backward_dx(*_gates_args(one, dtype=5)) == BAD_DTYPE
    for kw in (dict(B=0), dict(T=0), dict(N=-1), dict(G=0), dict(F=0), dict(Kin=0), dict(Kst=0)):
        assert lib.gcrnn_small_gates_backward_dx(*_gates_args(one, **kw)) == BAD_SHAPE, kw
    assert lib.gcrnn_small_gates_backward_dx(*_gates_args(one, G=65)) == UNSUPPORTED


def _nnz(N):
    return 6 * N          # about the density of the test graphs (4 N random edges, a hub, self-loops)


@pytest.mark.parametrize('dt,code', [(torch.float64, F64), (torch.float32, F32)])
def test_python_predicate_agrees_with_the_c_queries(dt, code, monkeypatch):
    monkeypatch.delenv('GCRNN_SMALL_GATHER', raising=False)
    lib = _lib.lib
    for N, G, F, Ki, Ks, gated in [(30, 2, 5, 3, 3, 0), (30, 2, 5, 3, 3, 1), (88, 8, 20, 4, 4, 0), (88, 8, 20, 5, 5, 0), (120, 1, 20, 5, 5, 1),
                                   (59, 1, 20, 4, 4, 1), (200, 1, 8, 3, 3, 0), (300, 2, 8, 6, 6, 0)]:
        train = bool(lib.gcrnn_small_supported(code, N, _nnz(N), G, F, Ki, Ks)) and \
            bool(lib.gcrnn_small_backward_supported(code, N, _nnz(N), G, F, Ki, Ks))
        if lib.gcrnn_small_dense_supported(code, N, G, F, Ki, Ks, 1, gated):
            want = train and bool(lib.gcrnn_small_dense_backward_dx_supported(code, N, G, F, Ki, Ks, gated))
        else:
            want = train                                       # the gather family: same LDS image as its plain backward
        assert ops.small_input_grad_supported(N, _nnz(N), G, F, Ki, Ks, dt, 1, gated=bool(gated)) == want, (N, G, F, Ki, Ks, gated)
        # the dx query never admits what the plain backward refuses
        assert lib.gcrnn_small_dense_backward_dx_supported(code, N, G, F, Ki, Ks, gated) <= lib.gcrnn_small_dense_supported(code, N, G, F, Ki, Ks, 1, gated)
    assert not ops.small_input_grad_supported(30, 90, 2, 5, 3, 3, torch.bfloat16)
    assert lib.gcrnn_small_dense_backward_dx_supported(7, 30, 2, 5, 3, 3, 0) == 0


DENSE_SHAPES = [(1, 1, 1, 1, 1, False, False), (30, 3, 20, 1, 1, False, False), (40, 2, 12, 5, 5, False, False), (40, 3, 12, 3, 2, True, True),
                (33, 2, 8, 2, 2, True, True), (65, 1, 33, 1, 1, True, False), (24, 63, 16, 2, 2, True, False), (20, 1, 8, 5, 5, True, False),
                (24, 2, 8, 2, 2, False, False), (30, 2, 5, 3, 3, True, True), (30, 5, 4, 3, 3, False, False), (88, 8, 20, 4, 4, False, False)]
GATHER_SHAPES = [(63, 2, 8, 1, 1, False), (64, 1, 32, 2, 2, False), (65, 1, 31, 3, 3, True), (69, 2, 30, 4, 4, False), (33, 3, 16, 5, 5, False),
                 (30, 2, 5, 3, 3, True)]


@pytest.mark.parametrize('dt', [torch.float64, torch.float32])
def test_predicate_accepts_the_tested_shapes_and_refuses_the_composed_ones(dt, monkeypatch):
    monkeypatch.delenv('GCRNN_SMALL_GATHER', raising=False)
    for N, G, F, Ki, Ks, gated, node in DENSE_SHAPES:
        assert ops.small_dense_supported(N, G, F, Ki, Ks, dt, backward=True, gated=gated), (N, G, F, Ki, Ks)
        assert ops.small_input_grad_supported(N, _nnz(N), G, F, Ki, Ks, dt, 1, gated=gated, node_gates=node), (N, G, F, Ki, Ks)
        if gated and not node:
            assert ops.small_gates_supported(N, G, F, Ki, Ks, dt, backward=True), (N, G, F, Ki, Ks)
    # the existing composed-* envelope cases stay on the composed path
    assert not ops.small_input_grad_supported(77, _nnz(77), 10, 65, 7, 7, dt)
    assert not ops.small_input_grad_supported(101, _nnz(101), 3, 63, 2, 2, dt, E=2)
    assert not ops.small_input_grad_supported(90, _nnz(90), 5, 64, 1, 1, dt, E=2, gated=True)
    assert not ops.small_input_grad_supported(1030, _nnz(1030), 4, 16, 3, 3, dt)
    assert not ops.small_input_grad_supported(1030, _nnz(1030), 9, 64, 7, 1, dt)
    # the matrix-core family's dx edge (fp64): one more tap per filter does not fit, the plain backward still does
    if dt == torch.float64:
        assert not ops.small_input_grad_supported(88, _nnz(88), 8, 20, 5, 5, dt)
        assert ops.small_training_supported(88, _nnz(88), 8, 20, 5, 5, dt) and ops.small_dense_supported(88, 8, 20, 5, 5, dt, True, False)
    monkeypatch.setenv('GCRNN_SMALL_GATHER', '1')
    for N, G, F, Ki, Ks, gated in GATHER_SHAPES:
        assert ops.small_input_grad_supported(N, _nnz(N), G, F, Ki, Ks, dt, 1, gated=gated), (N, G, F, Ki, Ks)
    assert not ops.small_input_grad_supported(40, _nnz(40), 3, 12, 3, 2, dt, 1, gated=True, node_gates=True)     # per-node gates: matrix cores only
    assert ops.small_input_grad_supported(512, 2336, 1, 5, 4, 4, dt)            # the family's LDS edge (fp64): five taps do not fit
    if dt == torch.float64:
        assert not ops.small_input_grad_supported(512, 2336, 1, 5, 5, 5, dt)
