"""Poisoned work buffers: every device buffer of the library comes from torch.empty, and most are larger than what the kernels write into
them (padded node rows, partly laid-out inputs, raw scratch, per-slot partial sums, rotating planes). A fresh process mostly gets zeroed
pages and a second run in one process gets the block the first run freed, so a kernel that reads what nobody wrote passes every test that
does not control what torch.empty returns. This module controls it.

poisoned_allocations(fill): for its duration torch.empty, torch.empty_like, torch.empty_strided and torch.Tensor.new_empty fill what they
return. assert_independent_of_workspace(build_and_run): the same problem under each fill gives finite and bit-identical results.

A plain helper module: no conftest, no pytest setting."""
import contextlib

import torch

FILLS = ('zero', 'nan', 'big')
BIG = 1.5 * 2.0 ** 100               # finite in bf16, fp32 and fp64; no weight of a test problem scales it away
_BIG_HALF = 1.5 * 2.0 ** 15          # (fp16 tops out at 65504: the package allocates none, the policy still covers it)
_BYTES = {'zero': 0x00, 'nan': 0xFF, 'big': 0x70}      # 0xFFFF / 0xFFFFFFFF / ...: NaN as bf16, fp32, fp64; 0x7070: 2.97e29 as bf16, as fp32
_NAMES = ('empty', 'empty_like', 'empty_strided')


class Counter(object):
    """What a poisoned_allocations block filled."""

    def __init__(self):
        self.tensors = 0
        self.bytes = 0

    def __repr__(self):
        return 'Counter(tensors=%d, bytes=%d)' % (self.tensors, self.bytes)


def _poisons(dtype):
    """Floating dtypes and uint8 (the package's two uint8 sites are raw work buffers that hold bf16). Every other integer dtype, bool
    and complex pass through: no pattern of ours can become an index or an address."""
    return dtype.is_floating_point or dtype == torch.uint8


def _fill(t, fill, counter):
    if not isinstance(t, torch.Tensor) or not _poisons(t.dtype) or t.numel() == 0:
        return t
    if t.is_cuda and torch.cuda.is_current_stream_capturing():       # captured graphs are out of scope
        return t
    d = t.detach()                                                   # (requires_grad=True: the fill is no part of any autograd graph)
    if t.dtype == torch.uint8:
        d.fill_(_BYTES[fill])
    elif fill == 'zero':
        d.zero_()
    elif fill == 'nan':
        d.fill_(float('nan'))
    else:
        d.fill_(_BIG_HALF if t.dtype == torch.float16 else BIG)
    counter.tensors += 1
    counter.bytes += t.numel() * t.element_size()
    return t


@contextlib.contextmanager
def poisoned_allocations(fill):
    """Replace the four allocation functions with wrappers that fill what they return; restore all four on exit, also after an exception.
    Yields the Counter. A call with out= returns what torch returns, untouched: that storage is the caller's."""
    assert fill in FILLS, fill
    counter = Counter()
    originals = {n: getattr(torch, n) for n in _NAMES}
    new_empty = torch.Tensor.new_empty
    own_new_empty = 'new_empty' in torch.Tensor.__dict__             # (it lives on the C base class: the patch shadows it, the restore un-shadows)

    def wrap(orig):
        def poisoned(*args, **kwargs):
            t = orig(*args, **kwargs)
            return t if kwargs.get('out') is not None else _fill(t, fill, counter)
        poisoned.__name__ = getattr(orig, '__name__', 'empty')
        poisoned.__wrapped__ = orig
        return poisoned

    def poisoned_new_empty(self, *args, **kwargs):
        return _fill(new_empty(self, *args, **kwargs), fill, counter)

    try:
        for n in _NAMES:
            setattr(torch, n, wrap(originals[n]))
        torch.Tensor.new_empty = poisoned_new_empty
        yield counter
    finally:
        for n in _NAMES:
            setattr(torch, n, originals[n])
        if own_new_empty:
            torch.Tensor.new_empty = new_empty
        elif 'new_empty' in torch.Tensor.__dict__:
            del torch.Tensor.new_empty


def _first_difference(a, b):
    """First index (row-major, in the tensor's own -- user -- coordinates) at which two tensors differ, NaN never equal to anything."""
    ne = (a != b) | a.isnan() | b.isnan() if a.is_floating_point() else (a != b)
    idx = torch.nonzero(ne.reshape(a.shape) if a.dim() else ne.reshape(1))
    return tuple(int(i) for i in idx[0]) if a.dim() else ()


def _snapshot(out):
    assert isinstance(out, dict) and out, 'build_and_run returns {name: tensor}, the semantic outputs'
    snap = {}
    for name, t in out.items():
        assert isinstance(t, torch.Tensor), (name, type(t))
        snap[name] = t.detach().cpu().clone()
    return snap


def assert_independent_of_workspace(build_and_run, fills=FILLS):
    """build_and_run() builds the whole problem from seeds (cell, graph operator, plans, inputs, optimiser state), runs the path and
    returns {name: tensor}: user-layout results in full, every gradient autograd returns, of a native-layout tensor the rows < N. It runs
    once under each fill; every output is finite, all runs are torch.equal name by name, and something was poisoned at all. Returns
    {fill: {name: tensor on the CPU}} for the caller's reference check."""
    from gated_gcrnns_amd import ops
    assert not ops._PACK_CACHE_ON[0], 'the packed-parameter cache is on: a run would start from an earlier run\'s packs'
    runs = {}
    for fill in fills:
        ops._PACK_CACHE.clear()
        with poisoned_allocations(fill) as counter:
            out = build_and_run()
            if torch.cuda.is_available() and torch.cuda.is_initialized():
                torch.cuda.synchronize()
        runs[fill] = _snapshot(out)
        assert counter.tensors > 0 and counter.bytes > 0, 'fill %r: the case allocated nothing through torch.empty -- a broken case' % fill
    first = runs[fills[0]]
    for fill in fills:
        assert runs[fill].keys() == first.keys(), (fill, sorted(runs[fill]), sorted(first))
        for name, t in runs[fill].items():
            if t.is_floating_point() and not bool(torch.isfinite(t).all()):
                bad = torch.nonzero(~torch.isfinite(t).reshape(t.shape if t.dim() else (1,)))[0]
                raise AssertionError('output %r is not finite under fill %r: first at index %s of shape %s (%d of %d elements)' % (
                    name, fill, tuple(int(i) for i in bad) if t.dim() else (), tuple(t.shape), int((~torch.isfinite(t)).sum()), t.numel()))
    for i, fa in enumerate(fills):
        for fb in fills[i + 1:]:
            for name in first:
                a, b = runs[fa][name], runs[fb][name]
                assert a.shape == b.shape and a.dtype == b.dtype, (name, fa, fb, a.shape, b.shape, a.dtype, b.dtype)
                if not torch.equal(a, b):
                    at = _first_difference(a, b)
                    va, vb = (a[at], b[at]) if a.dim() else (a, b)
                    ne = int(((a != b) | a.isnan() | b.isnan()).sum()) if a.is_floating_point() else int((a != b).sum())
                    raise AssertionError('output %r depends on what torch.empty returned: fills %r and %r differ first at index %s of shape %s '
                                         '(%r against %r; %d of %d elements differ)' % (name, fa, fb, at, tuple(a.shape), float(va), float(vb),
                                                                                        ne, a.numel()))
    return runs
