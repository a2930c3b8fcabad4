"""CPU: the host side of the small-graph node gates (gcrnn_small_node_gates_*) -- names in the header, the library and the ctypes table,
argument validation before any launch in the documented order, and the query: the drivers' shapes, what it must refuse, and that it never
admits what gcrnn_small_dense_supported(..., gated = 1) or the time gates' query refuses. No GPU compute is called."""
import ctypes as C
import itertools
import os
import re

import pytest
import torch

from conftest import ROOT
from gated_gcrnns_amd import _lib, ops

NEW = ('gcrnn_small_node_gates_supported', 'gcrnn_small_node_gates_forward', 'gcrnn_small_node_gates_backward',
       'gcrnn_small_node_gates_backward_dx')
OK, BAD_DTYPE, BAD_SHAPE, NULL, UNSUPPORTED = 0, 1, 2, 3, 4
F32, F64 = ops.dtype_code(torch.float32), ops.dtype_code(torch.float64)
DRIVERS = [(59, 1, 20, 4, 4), (80, 1, 20, 5, 5)]          # adj59 with K = 4 (epicenter), SBM 80 with K = 5 (k-step)


def test_new_names_are_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, 'include', 'gcrnn.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    declared = set(re.findall(r'\b(gcrnn_[a-z0-9_]+)\s*\(', txt))
    for n in NEW:
        assert n in declared, n
        assert n in _lib.EXPORTS, n
        assert hasattr(_lib.lib, n), n
    assert callable(ops.small_node_gates_supported) and callable(ops.small_node_gates)


def _args(n_ptr, last=None, dtype=F64, B=2, T=3, N=30, G=2, F=5, Kin=3, Kst=3, null_at=None, tail=()):
    """n_ptr pointers of which the optional ones may be NULL; null_at: index of a pointer to pass as NULL."""
    one = C.c_void_p(16)
    p = [one] * n_ptr
    if null_at is not None:
        p[null_at] = None
    return [dtype] + p + list(tail) + [B, T, N, G, F, Kin, Kst, None]


# (entry point, pointers, indices of the pointers that may be NULL)
ENTRIES = [('gcrnn_small_node_gates_forward', 9, (4, 6)),             # bias2, bf2
           ('gcrnn_small_node_gates_backward', 14, (4, 13)),          # bias2, pdh0
           ('gcrnn_small_node_gates_backward_dx', 15, (4, 13))]


@pytest.mark.parametrize('name,n_ptr,optional', ENTRIES, ids=[e[0] for e in ENTRIES])
def test_entry_points_validate_in_the_documented_order_before_any_launch(name, n_ptr, optional):
    fn = getattr(_lib.lib, name)
    for i in range(n_ptr):
        if i in optional:
            continue
        # a NULL pointer is reported first, whatever else is wrong
        assert fn(*_args(n_ptr, null_at=i)) == NULL, i
        assert fn(*_args(n_ptr, null_at=i, dtype=7, B=0, N=300)) == NULL, i
    assert fn(*_args(n_ptr, dtype=7)) == BAD_DTYPE
    assert fn(*_args(n_ptr, dtype=7, B=0, N=300)) == BAD_DTYPE                  # before the shape
    assert fn(*_args(n_ptr, dtype=ops.dtype_code(torch.bfloat16))) == BAD_DTYPE
    for kw in (dict(B=0), dict(T=0), dict(N=0), dict(G=-1), dict(F=0), dict(Kin=0), dict(Kst=-2)):
        assert fn(*_args(n_ptr, **kw)) == BAD_SHAPE, kw
    assert fn(*_args(n_ptr, B=0, N=300)) == BAD_SHAPE                            # before the query
    assert fn(*_args(n_ptr, N=300)) == UNSUPPORTED
    assert fn(*_args(n_ptr, G=65)) == UNSUPPORTED
    assert fn(*_args(n_ptr, Kin=9, Kst=9)) == UNSUPPORTED
    for i in optional:                                                            # optional pointers do not change the verdict
        assert fn(*_args(n_ptr, null_at=i, N=300)) == UNSUPPORTED, i


@pytest.mark.parametrize('dt,code', [(torch.float64, F64), (torch.float32, F32)], ids=['fp64', 'fp32'])
def test_query_accepts_both_drivers_shapes(dt, code, monkeypatch):
    monkeypatch.delenv('GCRNN_SMALL_GATHER', raising=False)
    for N, G, F, Ki, Ks in DRIVERS:
        for backward in (0, 1):
            assert _lib.lib.gcrnn_small_node_gates_supported(code, N, G, F, Ki, Ks, backward) == 1, (N, Ki, backward)
            assert ops.small_node_gates_supported(N, G, F, Ki, Ks, dt, backward=bool(backward)), (N, Ki, backward)


def test_query_refuses_what_it_must(monkeypatch):
    monkeypatch.delenv('GCRNN_SMALL_GATHER', raising=False)
    lib = _lib.lib
    N, G, F, Ki, Ks = DRIVERS[1]
    assert lib.gcrnn_small_node_gates_supported(ops.dtype_code(torch.bfloat16), N, G, F, Ki, Ks, 0) == 0
    assert lib.gcrnn_small_node_gates_supported(7, N, G, F, Ki, Ks, 0) == 0
    assert not ops.small_node_gates_supported(N, G, F, Ki, Ks, torch.bfloat16, backward=False)
    for code, dt in ((F32, torch.float32), (F64, torch.float64)):
        for backward in (0, 1):
            assert lib.gcrnn_small_node_gates_supported(code, 256, G, F, Ki, Ks, backward) == 0
            assert not ops.small_node_gates_supported(256, G, F, Ki, Ks, dt, backward=bool(backward))
            for bad in (dict(N=0), dict(G=0), dict(F=0), dict(Ki=0), dict(Ks=0), dict(Ki=9), dict(Ks=9), dict(G=65)):
                s = dict(N=N, G=G, F=F, Ki=Ki, Ks=Ks)
                s.update(bad)
                assert lib.gcrnn_small_node_gates_supported(code, s['N'], s['G'], s['F'], s['Ki'], s['Ks'], backward) == 0, bad
    # past the LDS rule: in fp64 the dense S of N = 150 alone (150 rows of >= 150 values) is 180 KB > 160 KB, whatever the rest is
    assert lib.gcrnn_small_node_gates_supported(F64, 150, 1, 4, 1, 1, 0) == 0
    monkeypatch.setenv('GCRNN_SMALL_GATHER', '1')
    for N_, G_, F_, Ki_, Ks_ in DRIVERS:
        for dt in (torch.float32, torch.float64):
            assert not ops.small_node_gates_supported(N_, G_, F_, Ki_, Ks_, dt, backward=False)
            assert not ops.small_node_gates_supported(N_, G_, F_, Ki_, Ks_, dt, backward=True)


GRID = list(itertools.product((1, 15, 16, 17, 33, 59, 80, 100, 120, 136, 160, 200, 256), (1, 3, 17, 64), (1, 5, 17, 20, 33, 64, 130),
                              ((1, 1), (1, 3), (3, 1), (2, 5), (5, 2), (4, 4), (8, 8))))


@pytest.mark.parametrize('code', [F64, F32], ids=['fp64', 'fp32'])
def test_query_never_admits_what_the_recurrence_or_the_gate_cell_refuses(code):
    lib = _lib.lib
    yes = 0
    for (N, G, F, (Ki, Ks)), backward in itertools.product(GRID, (0, 1)):
        if lib.gcrnn_small_node_gates_supported(code, N, G, F, Ki, Ks, backward):
            yes += 1
            assert lib.gcrnn_small_dense_supported(code, N, G, F, Ki, Ks, backward, 1) == 1, (N, G, F, Ki, Ks, backward)
            assert lib.gcrnn_small_gates_supported(code, N, G, F, Ki, Ks, backward) == 1, (N, G, F, Ki, Ks, backward)
    assert yes > 100          # the grid is not vacuous
