"""Self-test of the footprint arena (tests/_arena.py) on CPU tensors: a correct "kernel" passes, every kind of stray word is
detected and located, a word of the view left undefined is detected."""
import pytest
import torch

from _arena import SENTINEL_BITS, arena, flat_arena, guard_floats, sentinel

B, C, H, W, LD, C0 = 2, 12, 3, 5, 24, 8


def _ref():
    return torch.arange(B * C * H * W, dtype=torch.float32).view(B, C, H, W) + 1.0


def test_arena_layout_and_sentinel():
    from mydetection_amd import ops
    view, chk = arena(B, C, H, W, LD, C0, 'cpu')
    assert tuple(view.shape) == (B, C, H, W) and ops.nhwc_ld(view) == LD
    assert chk.guard >= max(W * LD, 4096) and guard_floats(W, LD) == 4096 and guard_floats(100, 64) == 6400
    assert chk.flat.numel() == 2 * chk.guard + B * H * W * LD
    assert bool((chk.flat.view(torch.int32) == SENTINEL_BITS).all())               # view included: an output arena
    assert torch.isnan(sentinel()) and int(sentinel().view(torch.int32)) == SENTINEL_BITS
    assert view.data_ptr() == chk.flat.data_ptr() + 4 * (chk.guard + C0)
    chk.outside_untouched()
    count, where = chk.undefined_in_view()
    assert count == B * C * H * W and where[0] == (0, 0, 0, C0)
    with pytest.raises(AssertionError, match='never written'):
        chk.view_defined()


def test_arena_correct_kernel_passes():
    for fill in ('sentinel', 'zero'):
        view, chk = arena(B, C, H, W, LD, C0, 'cpu', fill=fill)
        view.copy_(_ref())
        chk.view_defined()
        chk.outside_untouched()
        assert torch.equal(view, _ref())
    x, chk = arena(B, C, H, W, LD, C0, 'cpu', data=_ref())                         # input arena: data inside, poison around
    assert torch.equal(x, _ref())
    chk.outside_untouched()
    chk.view_defined()
    assert int((chk.body().view(torch.int32) == SENTINEL_BITS).sum()) == B * H * W * (LD - C)


@pytest.mark.parametrize('fill', ['sentinel', 'zero'])
@pytest.mark.parametrize('name', ['before_view', 'behind_last_channel', 'neighbour_interior', 'guard_lo', 'guard_hi',
                                  'guard_lo_first', 'guard_hi_last', 'nan_written'])
def test_arena_detects_and_locates_stray_word(name, fill):
    view, chk = arena(B, C, H, W, LD, C0, 'cpu', fill=fill)
    view.copy_(_ref())
    g, n = chk.guard, B * H * W * LD
    pix = (1 * H + 1) * W + 2                                                       # interior pixel (b 1, y 1, x 2)
    offset, want = {
        'before_view': (g + C0 - 1, ('pixel', 0, 0, 0, C0 - 1)),                    # the word just before the view's first
        'behind_last_channel': (g + (n - LD) + C0 + C, ('pixel', B - 1, H - 1, W - 1, C0 + C)),   # just behind the view's last
        'neighbour_interior': (g + pix * LD + C0 + C, ('pixel', 1, 1, 2, C0 + C)),
        'guard_lo': (g - 1, ('guard_lo', g - 1)),
        'guard_hi': (g + n, ('guard_hi', 0)),
        'guard_lo_first': (0, ('guard_lo', 0)),
        'guard_hi_last': (2 * g + n - 1, ('guard_hi', g - 1)),
        'nan_written': (g + pix * LD + C0 - 1, ('pixel', 1, 1, 2, C0 - 1)),
    }[name]
    chk.flat[offset] = float('nan') if name == 'nan_written' else 1.5              # a kernel's NaN is not the sentinel
    count, where = chk.changed_outside()
    assert count == 1 and where == [want]
    with pytest.raises(AssertionError, match='1 word'):
        chk.outside_untouched()
    chk.view_defined()                                                              # the view itself is whole


def test_arena_detects_undefined_and_non_finite_view_words():
    view, chk = arena(B, C, H, W, LD, C0, 'cpu', fill='zero')                       # zero surroundings: the view is poison all the same
    ref = _ref()
    view.copy_(ref)
    view[1, 5, 2, 3] = sentinel()
    count, where = chk.undefined_in_view()
    assert count == 1 and where == [(1, 2, 3, C0 + 5)]
    with pytest.raises(AssertionError, match='never written'):
        chk.view_defined()
    view[1, 5, 2, 3] = float('inf')
    assert chk.undefined_in_view()[0] == 0
    with pytest.raises(AssertionError, match='non-finite'):
        chk.view_defined()
    chk.outside_untouched()


def test_flat_arena():
    data = torch.arange(10, dtype=torch.float32)
    v, chk = flat_arena(10, 'cpu', data=data)
    assert torch.equal(v, data) and v.data_ptr() % 16 == 0
    chk.outside_untouched()
    v, chk = flat_arena(10, 'cpu')
    assert chk.undefined_in_view()[0] == 10
    v.copy_(data)
    chk.view_defined()
    chk.flat[chk.guard + 10] = 0.0                                                  # one float behind the 10
    assert chk.changed_outside() == (1, [('pixel', 0, 0, 0, 10)])


def test_misaligned_slice_is_not_a_view():
    """What the heads must respect: a channel range that starts off a 16-byte boundary is not a kernel-writable view."""
    from mydetection_amd import ops
    both, ld = ops.empty_nhwc(1, 86, 4, 4, 'cpu')
    assert ld == 88 and ops.nhwc_ld(both[:, 80:81]) == 88 and ops.nhwc_ld(both[:, 84:85]) == 88
    assert ops.nhwc_ld(both[:, 81:82]) is None
