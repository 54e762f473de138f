"""bk_multikrum_batch* (include/bk.h): the symbols are exported and the
argument checks answer without a GPU -- the shape checks come before anything
that needs a context."""
import pytest

from biscotti_amd import _lib

NAMES = ("bk_multikrum_batch_device", "bk_multikrum_batch", "bk_selection_margin_batch")


def _device(ctx, x, batch, n, d, ld, stride, f, sel=None):
    return _lib.lib().bk_multikrum_batch_device(ctx, x, _lib.BK_F64, batch, n, d, ld, stride, f,
                                                sel, None, None)


def _host(ctx, x, batch, n, d, ld, stride, f, sel=None):
    return _lib.lib().bk_multikrum_batch(ctx, x, _lib.BK_HOST, _lib.BK_F64, batch, n, d, ld,
                                         stride, f, sel, None, None, None)


def test_symbols_exported():
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert hasattr(L, name), name
    assert _lib.BK_MAX_BATCH == 65536


@pytest.mark.parametrize("entry", [_device, _host])
@pytest.mark.parametrize("batch,n,d,ld,stride,f,status,word", [
    (3, 10, 25, 25, 250, 2, _lib.BK_EINVAL, "null context"),      # valid shapes, no context
    (0, 10, 25, 25, 250, 2, _lib.BK_EINVAL, "batch"),
    (-1, 10, 25, 25, 250, 2, _lib.BK_EINVAL, "batch"),
    (3, 10, 25, 32, 9 * 32 + 25 - 1, 2, _lib.BK_EINVAL, "stride"),  # (n-1)*ld + d - 1
    (3, 10, 25, 25, 250, 0, _lib.BK_EINVAL, "f="),
    (3, 10, 25, 25, 250, 10, _lib.BK_EINVAL, "f="),
    (_lib.BK_MAX_BATCH + 1, 10, 25, 25, 250, 2, _lib.BK_ENOTSUP, "BK_MAX_BATCH"),
    (3, 10, 25, 24, 250, 2, _lib.BK_EINVAL, "ld="),
])
def test_argument_checks_need_no_gpu(entry, batch, n, d, ld, stride, f, status, word):
    assert entry(None, None, batch, n, d, ld, stride, f) == status
    assert word in _lib.last_error(), _lib.last_error()


def test_smallest_valid_stride_passes_the_shape_checks():
    """stride = (n-1)*ld + d is accepted: the next check (the context) answers"""
    assert _device(None, None, 3, 10, 25, 32, 9 * 32 + 25, 2) == _lib.BK_EINVAL
    assert "null context" in _lib.last_error()
    assert _device(None, None, _lib.BK_MAX_BATCH, 10, 25, 25, 250, 2) == _lib.BK_EINVAL
    assert "null context" in _lib.last_error()


def test_margin_batch_null_arguments():
    assert _lib.lib().bk_selection_margin_batch(None, None, 1) == _lib.BK_EINVAL
    assert _lib.last_error()


def test_krum_batch_clip_bounds():
    """krum's ValueError for clip outside [1, n), before any GPU work"""
    from biscotti_amd import krum_batch
    deltas = [[[float(i + j + b) for j in range(3)] for i in range(4)] for b in range(2)]
    for clip in (0, 4, -1, 5):
        with pytest.raises(ValueError):
            krum_batch(deltas, clip)
    with pytest.raises(ValueError):
        krum_batch(deltas[0], 1)  # one batch is not a sequence of batches
