"""CPU: the host side of the edge-gated small-graph input gradient -- gcrnn_small_edge_backward_dx in the header and the ctypes table,
its argument validation before any launch, ops.small_edge_input_grad_supported against small_edge_training_supported, and the module's
dispatch predicate under GCRNN_SMALL_EDGE_DX / GCRNN_NO_SMALL_EDGE. No GPU compute is called."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from gated_gcrnns_amd import _lib, ops
from gated_gcrnns_amd.graph import GraphOperator

NEW = 'gcrnn_small_edge_backward_dx'
F32, F64 = 0, 1                                       # dtype codes of include/gcrnn.h
NPTR = 34                                             # the 33 pointers of gcrnn_small_edge_backward, then dX
OPTIONAL = {6, 11, 12, 30, 31, 32}                    # bias, gi, gf, dgi, dgf, dh0
DX = 33


def gso_dir17():
    """Directed, signed weights; S[3][3] = -1 with row 3 otherwise empty (S + I cancels: an empty support row); node 5 isolated
    (its support is the self-loop of S + I alone); row 9 is a hub that reaches every node but the isolated one."""
    rng = np.random.default_rng(17)
    N = 17
    S = (rng.random((N, N)) < 0.2) * rng.uniform(0.2, 1.0, (N, N)) * rng.choice([-1.0, 1.0], (N, N))
    np.fill_diagonal(S, 0.0)
    S[9, :] = rng.uniform(0.2, 1.0, N) * rng.choice([-1.0, 1.0], N)
    S[3, :] = 0.0
    S[3, 3] = -1.0
    S[5, :] = 0.0
    S[:, 5] = 0.0
    S = S / np.abs(S).sum(axis=1).max()
    S[3, 3] = -1.0
    return S.reshape(1, N, N)


def gso_rand80():
    rng = np.random.default_rng(80)
    N = 80
    S = (rng.random((N, N)) < 0.1) * rng.uniform(0.1, 1.0, (N, N))
    np.fill_diagonal(S, 0.0)
    return (S / np.abs(S).sum(axis=1).max()).reshape(1, N, N)


def test_new_name_is_declared_and_bound():
    txt = open(os.path.join(ROOT, 'include', 'gcrnn.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    declared = set(re.findall(r'\b(gcrnn_[a-z0-9_]+)\s*\(', txt))
    assert NEW in declared
    assert NEW in _lib.EXPORTS
    assert hasattr(_lib.lib, NEW)
    assert len(getattr(_lib.lib, NEW).argtypes) == 1 + NPTR + 9 + 1                 # dtype, pointers, B .. nnz_support, stream
    assert len(_lib.lib.gcrnn_small_edge_backward.argtypes) == 1 + 33 + 9 + 1       # the plain entry keeps its signature
    assert 'gcrnn_small_edge_backward_dx_supported' not in declared               # the backward query answers for both
    assert callable(ops.small_edge_input_grad_supported)


def test_dx_entry_validates_before_launch():
    """Null pointer, bad shape, bad dtype and unsupported come back as status codes before anything is launched (the pointers here are
    host memory: a launch would be an error of its own). Same order and codes as gcrnn_small_edge_backward."""
    lib = _lib.lib
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    BAD_DTYPE, BAD_SHAPE, NULLP, UNSUPPORTED = (lib.gcrnn_status_string(c).decode() for c in (1, 2, 3, 4))

    def call(dtype=F64, ptrs=None, B=2, T=3, N=5, G=1, F=4, Kin=2, Kst=2, nnz=6, nnzs=9):
        ptrs = [p] * NPTR if ptrs is None else ptrs
        return lib.gcrnn_small_edge_backward_dx(dtype, *ptrs, B, T, N, G, F, Kin, Kst, nnz, nnzs, None)

    def name(status):
        return lib.gcrnn_status_string(status).decode()
    assert DX not in OPTIONAL
    for i in range(NPTR):
        if i in OPTIONAL:
            continue
        ptrs = [p] * NPTR
        ptrs[i] = None
        assert name(call(ptrs=ptrs)) == NULLP, i
    ptrs = [p] * NPTR
    ptrs[DX] = None                                                        # dX is required here, whatever else is wrong
    assert name(call(ptrs=ptrs, B=0, dtype=7)) == NULLP
    ptrs = [p] * NPTR
    ptrs[11] = None                                                        # gi without gf
    assert name(call(ptrs=ptrs)) == NULLP
    ptrs = [p] * NPTR
    ptrs[30] = None                                                        # gates without a place for their gradient
    assert name(call(ptrs=ptrs)) == NULLP
    ptrs = [p] * NPTR
    for i in OPTIONAL:
        ptrs[i] = None                                                     # all optional: the next check answers
    assert name(call(ptrs=ptrs, B=0)) == BAD_SHAPE
    assert name(call(T=0)) == BAD_SHAPE
    assert name(call(N=-1)) == BAD_SHAPE
    assert name(call(G=0)) == BAD_SHAPE
    assert name(call(Kin=0)) == BAD_SHAPE
    assert name(call(B=2 ** 31, T=2)) == BAD_SHAPE
    assert name(call(dtype=2)) == BAD_DTYPE
    assert name(call(dtype=7)) == BAD_DTYPE
    assert name(call(dtype=7, B=0)) == BAD_DTYPE                           # the dtype is looked at before the shape
    assert name(call(N=1000, F=20, nnz=5000, nnzs=6000)) == UNSUPPORTED
    assert name(call(N=80, F=32, Kin=3, Kst=3, nnz=640, nnzs=720)) == UNSUPPORTED      # fits the forward's LDS, not the backward's
    assert name(call(dtype=F32, N=1000, F=20, nnz=5000, nnzs=6000)) == UNSUPPORTED
    assert len({NULLP, BAD_SHAPE, BAD_DTYPE, UNSUPPORTED}) == 4


@pytest.mark.parametrize('dt', [torch.float64, torch.float32])
def test_predicate_is_the_training_predicate(dt):
    shapes = []
    for S, G, F, K in ((load_golden('g5_cls_T20K4_none')['S'], 1, 20, 4),              # adj59
                       (load_golden('g5_reg_multipMlp_none')['S'], 1, 20, 5),          # SBM50
                       (gso_rand80(), 1, 20, 3), (gso_rand80(), 1, 32, 3)):
        op = GraphOperator(S)
        shapes.append((S.shape[1], op.fwd[0].nnz, int(op.mask.nnz), G, F, K, K))
    for shape in shapes[:3]:
        assert ops.small_edge_input_grad_supported(*shape, dt), shape
    assert ops.small_edge_input_grad_supported(*shapes[3], dt) == (dt == torch.float32)           # 214 KiB of LDS in fp64
    shapes += [(1000, 10000, 11000, 1, 20, 4, 4), (200, 2000, 2200, 1, 64, 3, 3), (17, 60, 70, 9, 4, 2, 4)]
    for shape in shapes:
        assert ops.small_edge_input_grad_supported(*shape, dt) == ops.small_edge_training_supported(*shape, dt), shape
        assert ops.small_edge_input_grad_supported(*shape, dt) == \
            bool(_lib.lib.gcrnn_small_edge_backward_supported(ops.dtype_code(dt), *shape)), shape
    assert not ops.small_edge_input_grad_supported(*shapes[4], dt) and not ops.small_edge_input_grad_supported(*shapes[5], dt)
    assert not ops.small_edge_input_grad_supported(*shapes[0], torch.bfloat16)
    assert not ops.small_edge_input_grad_supported(*shapes[0], dt, E=2)


def test_dispatch_predicate_follows_the_environment(monkeypatch):
    """An X that wants a gradient takes the two-launch path only with GCRNN_SMALL_EDGE_DX=1; GCRNN_NO_SMALL_EDGE=1 wins; an X that alone
    wants one counts. The predicate reads the environment at every call and needs no device."""
    import gated_gcrnns_amd.Utils.graphML as gml
    monkeypatch.delenv('GCRNN_SMALL_EDGE_DX', raising=False)
    monkeypatch.delenv('GCRNN_NO_SMALL_EDGE', raising=False)
    S = gso_dir17()
    torch.manual_seed(6)
    cell = gml.GGCRNNCell(3, 7, 2, 2, torch.tanh, False, 'edge', 1, True)
    cell.addGSO(torch.tensor(S))
    cell = cell.double()
    X = torch.randn(2, 3, 3, 17, dtype=torch.float64, requires_grad=True)
    h0 = torch.zeros(2, 7, 17, dtype=torch.float64)
    assert cell._use_small_edge_training(X.detach(), h0)                   # as before: parameters want a gradient, X does not
    assert not cell._use_small_edge_training(X, h0)
    monkeypatch.setenv('GCRNN_SMALL_EDGE_DX', '1')
    assert cell._use_small_edge_training(X, h0)
    assert cell._use_small_edge_training(X.detach(), h0)
    assert not cell._use_small_edge(X, h0)                                 # never the inference path
    with torch.no_grad():
        assert not cell._use_small_edge_training(X, h0)
    monkeypatch.setenv('GCRNN_NO_SMALL_EDGE', '1')
    assert not cell._use_small_edge_training(X, h0)
    monkeypatch.delenv('GCRNN_NO_SMALL_EDGE')
    for p in cell.parameters():
        p.requires_grad_(False)
    assert cell._use_small_edge_training(X, h0)                            # X alone
    assert not cell._use_small_edge_training(X.detach(), h0)               # nothing wants a gradient
    monkeypatch.delenv('GCRNN_SMALL_EDGE_DX')
    assert not cell._use_small_edge_training(X, h0)
