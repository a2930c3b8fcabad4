"""CPU: argument validation of gcrnn_small_dense_forward and gcrnn_small_dense_backward, the two matrix-core small-graph entry points
without a dtype check of their own (an unknown dtype, like a shape outside the envelope, is UNSUPPORTED there). Dummy pointers and never a
fully valid call: a call that got as far as a launch would fault, so a status code back is the proof. The order of the checks is part of
the contract: NULL pointers, then B / T, then the support query. No GPU compute is called."""
import ctypes as C

import torch

from gated_gcrnns_amd import _lib, ops

OK, BAD_DTYPE, BAD_SHAPE, NULL, UNSUPPORTED = 0, 1, 2, 3, 4
F32, F64, BF16 = ops.dtype_code(torch.float32), ops.dtype_code(torch.float64), ops.dtype_code(torch.bfloat16)
ONE = C.c_void_p(16)


def _fwd_args(dtype=F64, B=2, T=3, N=30, G=2, F=5, Kin=3, Kst=3, **ptr):
    names = ('X', 'h0', 'wA', 'wB', 'bias', 'gi', 'gf', 'Sdense', 'H')
    p = {n: ONE for n in names}
    p['gi'] = p['gf'] = None
    p.update(ptr)
    return [dtype] + [p[n] for n in names] + [B, T, N, G, F, Kin, Kst, 0, 0, 0, None]


def _bwd_args(dtype=F64, B=2, T=3, N=30, G=2, F=5, Kin=3, Kst=3, **ptr):
    names = ('X', 'h0', 'H', 'dH', 'wA', 'wB', 'bias', 'gi', 'gf', 'Sdense', 'pA', 'pB', 'pb', 'dgi', 'dgf', 'dh0')
    p = {n: ONE for n in names}
    p['gi'] = p['gf'] = p['dgi'] = p['dgf'] = None
    p.update(ptr)
    return [dtype] + [p[n] for n in names] + [B, T, N, G, F, Kin, Kst, 0, 0, 0, None]


def test_the_default_arguments_are_inside_the_envelope():
    """Every case below is one step away from a valid call, not two: the support query says yes to the defaults."""
    q = _lib.lib.gcrnn_small_dense_supported
    for code in (F32, F64):
        for backward in (0, 1):
            for gated in (0, 1):
                assert q(code, 30, 2, 5, 3, 3, backward, gated) == 1


def test_forward_validates_before_launch():
    f = _lib.lib.gcrnn_small_dense_forward
    for n in ('X', 'h0', 'wA', 'wB', 'Sdense', 'H'):
        assert f(*_fwd_args(**{n: None})) == NULL, n
    assert f(*_fwd_args(gi=ONE)) == NULL                                           # one gate without the other
    assert f(*_fwd_args(gf=ONE)) == NULL
    for kw in (dict(B=0), dict(T=0), dict(B=-1), dict(T=-2), dict(B=2 ** 31)):
        assert f(*_fwd_args(**kw)) == BAD_SHAPE, kw
    for code in (F32, F64):
        assert f(*_fwd_args(dtype=code, N=0)) == UNSUPPORTED
        assert f(*_fwd_args(dtype=code, N=300)) == UNSUPPORTED
    assert f(*_fwd_args(dtype=BF16)) == UNSUPPORTED                                # no BAD_DTYPE from this entry
    assert f(*_fwd_args(dtype=9)) == UNSUPPORTED
    assert f(*_fwd_args(gi=ONE, gf=ONE, N=300)) == UNSUPPORTED
    # the order of the checks
    assert f(*_fwd_args(X=None, B=0, dtype=BF16)) == NULL
    assert f(*_fwd_args(T=0, dtype=BF16)) == BAD_SHAPE
    assert f(*_fwd_args(B=0, N=300)) == BAD_SHAPE


def test_backward_validates_before_launch():
    f = _lib.lib.gcrnn_small_dense_backward
    for n in ('X', 'h0', 'H', 'dH', 'wA', 'wB', 'Sdense', 'pA', 'pB', 'pb'):
        assert f(*_bwd_args(**{n: None})) == NULL, n
    assert f(*_bwd_args(gi=ONE)) == NULL                                           # one gate without the other
    assert f(*_bwd_args(gf=ONE, dgi=ONE, dgf=ONE)) == NULL
    assert f(*_bwd_args(gi=ONE, gf=ONE)) == NULL                                   # gates without room for their gradients
    assert f(*_bwd_args(gi=ONE, gf=ONE, dgi=ONE)) == NULL
    assert f(*_bwd_args(gi=ONE, gf=ONE, dgf=ONE)) == NULL
    for kw in (dict(B=0), dict(T=0), dict(B=-1), dict(T=-2), dict(B=2 ** 31)):
        assert f(*_bwd_args(**kw)) == BAD_SHAPE, kw
    for code in (F32, F64):
        assert f(*_bwd_args(dtype=code, N=0)) == UNSUPPORTED
        assert f(*_bwd_args(dtype=code, N=300)) == UNSUPPORTED
    assert f(*_bwd_args(dtype=BF16)) == UNSUPPORTED                                # no BAD_DTYPE from this entry
    assert f(*_bwd_args(dtype=9)) == UNSUPPORTED
    assert f(*_bwd_args(gi=ONE, gf=ONE, dgi=ONE, dgf=ONE, N=300)) == UNSUPPORTED
    assert f(*_bwd_args(dh0=None, N=300)) == UNSUPPORTED                           # (dh0 may be NULL)
    # the order of the checks
    assert f(*_bwd_args(pb=None, T=0, dtype=BF16)) == NULL
    assert f(*_bwd_args(gi=ONE, gf=ONE, B=0)) == NULL
    assert f(*_bwd_args(B=0, dtype=BF16)) == BAD_SHAPE
    assert f(*_bwd_args(T=0, N=300)) == BAD_SHAPE
