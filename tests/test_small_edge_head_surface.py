"""CPU: the host side of the edge-gated small-graph heads -- gcrnn_small_edge_head_supported, gcrnn_small_edge_forward_head and
gcrnn_small_edge_backward_head in the header and the ctypes table, the query without a device, the entries' argument validation before
any launch, and the public ops names. No GPU compute is called."""
import ctypes as C
import os
import re

import torch

from conftest import ROOT, load_golden
from gated_gcrnns_amd import _lib, ops
from gated_gcrnns_amd.graph import GraphOperator
from test_small_edge_input_grad_surface import gso_rand80

NEW = ('gcrnn_small_edge_head_supported', 'gcrnn_small_edge_forward_head', 'gcrnn_small_edge_backward_head')
F32, F64, BF16 = 0, 1, 2                              # dtype codes of include/gcrnn.h
LAST, NODE = 1, 2                                     # GCRNN_SMALL_EDGE_HEAD_*
ALL, ONLY_LAST, NONE = 0, 1, 2                        # GCRNN_SMALL_STATES_*
FWD_NPTR = 24                                         # the 21 pointers of gcrnn_small_edge_forward, then head_w, head_b, Y
FWD_OPTIONAL = {4, 9, 10, 22}                         # bias, gi, gf, head_b
FWD_H = 20
BWD_NPTR = 35                                         # X, h0, H, up, head_w, then gcrnn_small_edge_backward_dx's from wA on
BWD_OPTIONAL = {7, 12, 13, 31, 32, 33, 34}            # bias, gi, gf, dgi, dgf, dh0, dX


def _driver_shapes():
    out = []
    for S, G, F, K in ((load_golden('g5_cls_T20K4_none')['S'], 1, 20, 4),              # adj59, the epicenter driver
                       (load_golden('g5_reg_multipMlp_none')['S'], 1, 20, 5)):         # SBM 50, the k-step driver
        op = GraphOperator(S)
        out.append((S.shape[1], op.fwd[0].nnz, int(op.mask.nnz), G, F, K, K))
    return out


def test_new_names_are_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, 'include', 'gcrnn.h')).read()
    assert 'architectures.py:1616-1627' in txt and 'architectures.py:1844-1856' in txt
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    declared = set(re.findall(r'\b(gcrnn_[a-z0-9_]+)\s*\(', txt))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(_lib.lib, name), name
    assert len(_lib.lib.gcrnn_small_edge_head_supported.argtypes) == 11
    assert len(_lib.lib.gcrnn_small_edge_forward_head.argtypes) == 1 + FWD_NPTR + 10 + 2 + 1      # dtype, pointers, B .. NC, kind, store, stream
    assert len(_lib.lib.gcrnn_small_edge_backward_head.argtypes) == 1 + BWD_NPTR + 10 + 1 + 1     # dtype, pointers, B .. NC, kind, stream
    # the existing entries keep their signatures
    assert len(_lib.lib.gcrnn_small_edge_forward.argtypes) == 1 + 21 + 9 + 1 + 1
    assert len(_lib.lib.gcrnn_small_edge_backward.argtypes) == 1 + 33 + 9 + 1
    assert len(_lib.lib.gcrnn_small_edge_backward_dx.argtypes) == 1 + 34 + 9 + 1
    for name in ('small_edge_head_supported', 'small_edge_cell_classify', 'small_edge_cell_regress', '_SmallEdgeCellHead',
                 '_SmallEdgeCellNodeHead'):
        assert hasattr(ops, name), name
    assert (ops.SMALL_EDGE_HEAD_LAST, ops.SMALL_EDGE_HEAD_NODE) == (LAST, NODE)


def test_query_answers_without_a_device():
    q = _lib.lib.gcrnn_small_edge_head_supported
    for shape in _driver_shapes():
        for dt in (F32, F64):
            for backward in (0, 1):
                assert q(dt, *shape, LAST, 11, backward) == 1, (shape, dt, backward)
                assert q(dt, *shape, NODE, 1, backward) == 1 and q(dt, *shape, NODE, 8, backward) == 1, (shape, dt, backward)
    shape = _driver_shapes()[0]
    assert q(BF16, *shape, LAST, 11, 0) == 0 and q(BF16, *shape, NODE, 1, 0) == 0
    assert q(F64, *shape, LAST, 0, 0) == 0 and q(F64, *shape, NODE, 0, 0) == 0
    assert q(F64, *shape, NODE, 9, 0) == 0 and q(F32, *shape, NODE, 9, 1) == 0
    for kind in (0, 3, -1):
        assert q(F64, *shape, kind, 1, 0) == 0
    assert q(F32, 129, 1000, 1100, 1, 4, 2, 2, LAST, 3, 0) == 0 and q(F32, 129, 1000, 1100, 1, 4, 2, 2, NODE, 1, 0) == 0
    assert q(F32, 128, 1000, 1100, 1, 4, 2, 2, LAST, 3, 1) == 1
    for dt in (torch.float32, torch.float64):
        assert ops.small_edge_head_supported(*shape, LAST, 11, dt, True) and ops.small_edge_head_supported(*shape, NODE, 1, dt, False)
        assert not ops.small_edge_head_supported(*shape, NODE, 1, dt, False, E=2)
    assert not ops.small_edge_head_supported(*shape, LAST, 11, torch.bfloat16, False)


def test_query_never_admits_more_than_the_plain_edge_queries():
    q = _lib.lib.gcrnn_small_edge_head_supported
    fwd, bwd = _lib.lib.gcrnn_small_edge_supported, _lib.lib.gcrnn_small_edge_backward_supported
    op = GraphOperator(gso_rand80())
    nnz, nnzs = op.fwd[0].nnz, int(op.mask.nnz)
    shapes = _driver_shapes() + [(80, nnz, nnzs, 1, 32, 3, 3), (80, nnz, nnzs, 1, 20, 3, 3), (17, 60, 70, 9, 4, 2, 4),
                                 (1000, 10000, 11000, 1, 20, 4, 4), (200, 2000, 2200, 1, 64, 3, 3), (128, 1000, 1100, 1, 30, 2, 2),
                                 (128, 1000, 1100, 1, 31, 2, 2)]
    # both sides of the LDS edge of the forward and of the backward: F grows at N = 80, K = 3 until neither fits
    shapes += [(80, nnz, nnzs, 1, F, 3, 3) for F in range(20, 52, 2)]
    seen = set()
    for shape in shapes:
        for dt in (F32, F64):
            for kind, NC in ((LAST, 11), (NODE, 1), (NODE, 8)):
                a0, a1 = q(dt, *shape, kind, NC, 0), q(dt, *shape, kind, NC, 1)
                assert a0 <= fwd(dt, *shape) and a1 <= min(fwd(dt, *shape), bwd(dt, *shape)), (shape, dt, kind, NC)
                assert a1 <= a0
                seen.add((fwd(dt, *shape), bwd(dt, *shape), a0, a1))
    assert q(F64, 80, nnz, nnzs, 1, 32, 3, 3, NODE, 1, 0) == 1 and q(F64, 80, nnz, nnzs, 1, 32, 3, 3, NODE, 1, 1) == 0    # the backward refuses
    assert q(F32, 80, nnz, nnzs, 1, 32, 3, 3, LAST, 11, 1) == 1
    assert {(1, 1, 1, 1), (1, 0, 1, 0), (0, 0, 0, 0)} <= seen


def _names(lib):
    return tuple(lib.gcrnn_status_string(c).decode() for c in (1, 2, 3, 4))


def test_forward_head_validates_before_launch():
    """Status codes come back before anything is launched (the pointers are host memory: a launch would be an error of its own)."""
    lib = _lib.lib
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    BAD_DTYPE, BAD_SHAPE, NULLP, UNSUPPORTED = _names(lib)

    def call(dtype=F64, ptrs=None, B=2, T=3, N=5, G=1, F=4, Kin=2, Kst=2, nnz=6, nnzs=9, NC=3, kind=LAST, store=ALL):
        ptrs = [p] * FWD_NPTR if ptrs is None else ptrs
        return lib.gcrnn_status_string(lib.gcrnn_small_edge_forward_head(dtype, *ptrs, B, T, N, G, F, Kin, Kst, nnz, nnzs, NC, kind, store,
                                                                         None)).decode()
    for kind in (LAST, NODE):
        for i in range(FWD_NPTR):
            if i in FWD_OPTIONAL:
                continue
            ptrs = [p] * FWD_NPTR
            ptrs[i] = None
            assert call(ptrs=ptrs, kind=kind, B=0, dtype=7) == NULLP, i              # a required pointer, whatever else is wrong
    ptrs = [p] * FWD_NPTR
    ptrs[FWD_H] = None
    for kind in (LAST, NODE):
        assert call(ptrs=ptrs, kind=kind, store=ALL) == NULLP and call(ptrs=ptrs, kind=kind, store=ONLY_LAST) == NULLP
        assert call(ptrs=ptrs, kind=kind, store=NONE, B=0) == BAD_SHAPE             # H = NULL goes with STATES_NONE only: the next check answers
    ptrs = [p] * FWD_NPTR
    ptrs[9] = None                                                                  # gi without gf
    assert call(ptrs=ptrs) == NULLP
    ptrs = [p] * FWD_NPTR
    for i in FWD_OPTIONAL:
        ptrs[i] = None
    assert call(ptrs=ptrs, T=0) == BAD_SHAPE
    assert call(dtype=BF16) == BAD_DTYPE and call(dtype=7, B=0) == BAD_DTYPE         # the dtype is looked at before the shape
    assert call(N=-1) == BAD_SHAPE and call(Kst=0) == BAD_SHAPE
    assert call(B=2 ** 31, T=2) == BAD_SHAPE and call(B=2 ** 16, T=2 ** 16) == BAD_SHAPE
    for store in (-1, 3):
        assert call(store=store) == BAD_SHAPE
    for kind in (0, 3):
        assert call(kind=kind) == BAD_SHAPE
    assert call(NC=0) == BAD_SHAPE and call(kind=NODE, NC=9) == BAD_SHAPE and call(kind=NODE, NC=0) == BAD_SHAPE
    assert call(N=1000, F=20, nnz=5000, nnzs=6000) == UNSUPPORTED
    assert call(dtype=F32, kind=NODE, NC=1, N=129, nnz=500, nnzs=600) == UNSUPPORTED
    assert len({NULLP, BAD_SHAPE, BAD_DTYPE, UNSUPPORTED}) == 4


def test_backward_head_validates_before_launch():
    lib = _lib.lib
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    BAD_DTYPE, BAD_SHAPE, NULLP, UNSUPPORTED = _names(lib)

    def call(dtype=F64, ptrs=None, B=2, T=3, N=5, G=1, F=4, Kin=2, Kst=2, nnz=6, nnzs=9, NC=3, kind=LAST):
        ptrs = [p] * BWD_NPTR if ptrs is None else ptrs
        return lib.gcrnn_status_string(lib.gcrnn_small_edge_backward_head(dtype, *ptrs, B, T, N, G, F, Kin, Kst, nnz, nnzs, NC, kind,
                                                                          None)).decode()
    for kind in (LAST, NODE):
        for i in range(BWD_NPTR):
            if i in BWD_OPTIONAL:
                continue
            ptrs = [p] * BWD_NPTR
            ptrs[i] = None
            assert call(ptrs=ptrs, kind=kind, B=0, dtype=7) == NULLP, i
    ptrs = [p] * BWD_NPTR
    ptrs[12] = None                                                                 # gi without gf
    assert call(ptrs=ptrs) == NULLP
    ptrs = [p] * BWD_NPTR
    ptrs[31] = None                                                                 # gates without a place for their gradient
    assert call(ptrs=ptrs) == NULLP
    ptrs = [p] * BWD_NPTR
    for i in BWD_OPTIONAL:
        ptrs[i] = None                                                              # dX among them: NULL selects the plain input branch
    assert call(ptrs=ptrs, B=0) == BAD_SHAPE
    assert call(dtype=BF16) == BAD_DTYPE and call(dtype=7, B=0) == BAD_DTYPE
    assert call(T=0) == BAD_SHAPE and call(G=0) == BAD_SHAPE and call(B=2 ** 31, T=2) == BAD_SHAPE
    for kind in (0, 3):
        assert call(kind=kind) == BAD_SHAPE
    assert call(NC=0) == BAD_SHAPE and call(kind=NODE, NC=9) == BAD_SHAPE
    assert call(N=1000, F=20, nnz=5000, nnzs=6000) == UNSUPPORTED
    assert call(N=80, F=32, Kin=3, Kst=3, nnz=640, nnzs=720) == UNSUPPORTED          # fits the forward's LDS, not the backward's
    assert call(dtype=F32, N=80, F=32, Kin=3, Kst=3, nnz=640, nnzs=720, B=0) == BAD_SHAPE
    assert len({NULLP, BAD_SHAPE, BAD_DTYPE, UNSUPPORTED}) == 4


def test_dispatch_is_opt_in_and_the_off_switches_win(monkeypatch):
    """GGCRNNCell.classify / regress decline for an edge-gated cell unless GCRNN_SMALL_EDGE_HEAD is set; read at every call; no device."""
    import gated_gcrnns_amd.Utils.graphML as gml
    from test_small_edge_input_grad_surface import gso_dir17
    for v in ('GCRNN_SMALL_EDGE_HEAD', 'GCRNN_NO_SMALL_EDGE', 'GCRNN_NO_SMALL_HEAD', 'GCRNN_NO_SMALL_NODE_HEAD', 'GCRNN_SMALL_EDGE_DX'):
        monkeypatch.delenv(v, raising=False)
    torch.manual_seed(6)
    cell = gml.GGCRNNCell(3, 7, 2, 2, torch.tanh, False, 'edge', 1, True)
    cell.addGSO(torch.tensor(gso_dir17()))
    cell = cell.double()
    X = torch.randn(2, 3, 3, 17, dtype=torch.float64)
    h0 = torch.zeros(2, 7, 17, dtype=torch.float64)
    calls = []
    monkeypatch.setattr(ops, 'small_edge_cell_classify', lambda *a, **k: calls.append('classify') or 'C')
    monkeypatch.setattr(ops, 'small_edge_cell_regress', lambda *a, **k: calls.append('regress') or 'R')
    monkeypatch.setattr(ops, 'require_device', lambda *a: None)
    hw, nw = torch.randn(5, 7 * 17, dtype=torch.float64), torch.randn(2, 7, dtype=torch.float64)
    assert cell.classify(X, h0, hw, None) is None and cell.regress(X, h0, nw, None) is None and calls == []
    monkeypatch.setenv('GCRNN_SMALL_EDGE_HEAD', '1')
    assert cell.classify(X, h0, hw, None) == 'C'
    assert cell.regress(X, h0, nw, None) is None                                   # the fp64 per-node head is off the dispatch (_small_edge_head_pays)
    assert not cell._small_edge_head_pays(X, ops.SMALL_EDGE_HEAD_NODE) and cell._small_edge_head_pays(X, ops.SMALL_EDGE_HEAD_LAST)
    assert cell._small_edge_head_pays(X.float(), ops.SMALL_EDGE_HEAD_NODE)
    monkeypatch.setenv('GCRNN_SMALL_EDGE_HEAD', 'all')                             # ... unless every supported row is asked for
    assert cell.classify(X, h0, hw, None) == 'C' and cell.regress(X, h0, nw, None) == 'R'
    with torch.no_grad():
        assert cell.classify(X, h0, hw, None) == 'C' and cell.regress(X, h0, nw, None) == 'R'
    assert cell.classify(X, h0, hw.float(), None) is None                          # a head in another dtype
    assert cell.classify(X, h0, hw[:, :-1], None) is None                          # ... of another width
    assert cell.regress(X, h0, torch.randn(9, 7, dtype=torch.float64), None) is None           # O = 9
    assert cell.regress(X.requires_grad_(True), h0, nw, None) is None              # an X that wants a gradient: GCRNN_SMALL_EDGE_DX's rule
    monkeypatch.setenv('GCRNN_SMALL_EDGE_DX', '1')
    assert cell.regress(X, h0, nw, None) == 'R'
    X = X.detach()
    for off, fn, w in (('GCRNN_NO_SMALL_EDGE', cell.classify, hw), ('GCRNN_NO_SMALL_EDGE', cell.regress, nw),
                       ('GCRNN_NO_SMALL_HEAD', cell.classify, hw), ('GCRNN_NO_SMALL_NODE_HEAD', cell.regress, nw)):
        monkeypatch.setenv(off, '1')
        assert fn(X, h0, w, None) is None, off
        monkeypatch.delenv(off)
        assert fn(X, h0, w, None) is not None
    monkeypatch.setenv('GCRNN_NO_SMALL_HEAD', '1')                                  # each head's own switch, not the other's
    assert cell.regress(X, h0, nw, None) == 'R'
