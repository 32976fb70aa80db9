"""GPU tests of the one path behind every per-stream state (mydetection_amd/ops.py: _state_new, _state_reset): for the tracker,
the zones, the trails, the camera motion and the appearance, a fresh state equals -- with == on every word, padding included --
a buffer of another content that went through the family's reset, and its field views have the shapes their docstrings state.
The smallest legal sizes, and no launch but the resets."""
import pytest
import torch

pytestmark = pytest.mark.gpu

S, MT, L, HW = 2, 5, 2, (48, 64)                                     # max_tracks = 5: every slot family ends in padding words
I32, I64, F32, U8 = torch.int32, torch.int64, torch.float32, torch.uint8
# 48x64 frames reduced by 2 with search 4: 24x32 reduced pixels, one 16x16 block, 16x16 patches
VIEWS = {
    'track': {'x': ((S, 5, MT), F32), 'v': ((S, 5, MT), F32), 'pxx': ((S, 5, MT), F32), 'pxv': ((S, 5, MT), F32), 'pvv': ((S, 5, MT), F32),
              'score': ((S, MT), F32), 'cls': ((S, MT), I64), 'id': ((S, MT), I64), 'missed': ((S, MT), I32), 'next_id': ((S,), I64),
              'live': ((S,), I32)},
    'zones': {'now': ((S,), I32), 'zone_counts': ((S, 16, 4), I32), 'line_counts': ((S, 16, 2), I32), 'dwell_max': ((S, 16), I32),
              'dwell_sum': ((S, 16), I64), 'id': ((S, MT), I64), 'inside': ((S, MT), I32), 'sides': ((S, MT), I32), 'px': ((S, MT), I32),
              'py': ((S, MT), I32), 'entered': ((S, 16, MT), I32)},
    'trails': {'id': ((S, MT), I64), 'fill': ((S, MT), I32), 'head': ((S, MT), I32), 'ring': ((S, MT, L, 2), I32)},
    'motion': {'seen': ((S,), I32), 'reduced': ((S, 24, 32), U8), 'patches': ((S, 1, 16, 16), U8)},
    'appear': {'has': ((S, MT), I32), 'tmpl': ((S, 128, MT), I32)},
}


def _args(name):
    from mydetection_amd import ops
    if name == 'motion':
        return HW, ops.motion_set(reduce=2, search=4)
    return (MT, L) if name == 'trails' else (MT,)


@pytest.mark.parametrize('name', sorted(VIEWS))
def test_fresh_state_is_a_reset_one(name):
    from mydetection_amd import ops
    args = _args(name)
    fresh = getattr(ops, f'{name}_state')(S, *args, 'cuda')
    assert fresh.dtype == I32 and fresh.dim() == 2 and fresh.shape[0] == S and fresh.is_contiguous() and fresh.is_cuda
    if name != 'motion':
        words = getattr(ops, f'{name}_state_words')(*args)
        assert fresh.shape[1] == words and words % 4 == 0
        lib = ops._lib
        raw = {'track': lib.TRACK_STATE_HEADER + lib.TRACK_SLOT_WORDS * MT, 'zones': lib.ZONES_STATE_HEADER + lib.ZONES_SLOT_WORDS * MT,
               'trails': MT * (4 + 2 * L), 'appear': (1 + lib.APPEAR_BINS) * MT}[name]
        assert words == (raw + 3) // 4 * 4 and (raw % 4 or name == 'trails'), 'the row ends in padding words (trails: 40 words, none)'
    used = torch.full_like(fresh, 0x5A5A5A5A)
    assert getattr(ops, f'{name}_reset_')(used, *args) is used
    assert torch.equal(used, fresh), f'{int((used != fresh).sum())} words differ'
    views = getattr(ops, f'{name}_state_views')(fresh, *args)
    assert {k: (tuple(t.shape), t.dtype) for k, t in views.items()} == VIEWS[name]
    host = getattr(ops, f'{name}_state_views')(fresh.cpu(), *args)   # the views work on a host copy too
    assert all(torch.equal(host[k], views[k].cpu()) for k in views)
