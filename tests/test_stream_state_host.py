"""Host tests of the rules every per-stream state shares (mydetection_amd/ops.py: _StateFamily, _state_check, _state_reset,
_state_new, out_planes): the tracker, the zones, the trails, the camera motion and the appearance state go through ONE statement
of each rule, and these tests hold all five to it.  No device is touched: every refusal comes before a launch."""
import pytest
import torch

FAMILIES = ('track', 'zones', 'trails', 'motion', 'appear')
SLOT_FAMILIES = ('track', 'zones', 'trails', 'appear')               # a state of max_tracks slots per stream
MT, L, HW = 5, 2, (48, 64)


def _family(name, max_tracks=MT):
    """(new(streams, device), reset_(state), words) of a family at the sizes of this file."""
    from mydetection_amd import ops
    if name == 'motion':
        args = (HW, ops.motion_set(reduce=2, search=4))
        words = lambda: ops.motion_geometry(*args)['state_words']
    else:
        args = (max_tracks, L) if name == 'trails' else (max_tracks,)
        words = lambda: getattr(ops, f'{name}_state_words')(*args)
    new, reset = getattr(ops, f'{name}_state'), getattr(ops, f'{name}_reset_')
    return (lambda streams, device='cpu': new(streams, *args, device)), (lambda state: reset(state, *args)), words


@pytest.mark.parametrize('name', FAMILIES)
def test_no_streams_is_refused(name):
    new, _, _ = _family(name)
    for streams in (0, -1):
        with pytest.raises(ValueError, match='streams'):
            new(streams)


@pytest.mark.parametrize('name', SLOT_FAMILIES)
@pytest.mark.parametrize('max_tracks', (0, 513))
def test_max_tracks_range(name, max_tracks):
    new, reset, words = _family(name, max_tracks)
    with pytest.raises(ValueError, match='max_tracks'):
        words()
    with pytest.raises(ValueError, match='max_tracks'):
        new(2)
    with pytest.raises(ValueError, match='max_tracks'):
        reset(torch.zeros((2, 8), dtype=torch.int32))


@pytest.mark.parametrize('name', FAMILIES)
def test_reset_refuses_what_is_no_state(name):
    """Every tensor below is on the host: the ValueError of the state rule wins over the RuntimeError of the device rule."""
    _, reset, words = _family(name)
    w = words()
    assert w % 4 == 0 and w > 4
    for bad in (torch.zeros((2, w - 4), dtype=torch.int32), torch.zeros((2, w), dtype=torch.int64),
                torch.zeros((2, 2 * w), dtype=torch.int32)[:, ::2], torch.zeros((w,), dtype=torch.int32), None):
        with pytest.raises(ValueError, match='state'):
            reset(bad)


@pytest.mark.parametrize('name', FAMILIES)
def test_host_state(name):
    """A correct state on the host: the four families with a reset kernel have no CPU path, the appearance state is cleared."""
    new, reset, words = _family(name)
    state = torch.full((2, words()), 0x5A5A5A5A, dtype=torch.int32)
    if name == 'appear':
        assert reset(state) is state and not state.any()
        fresh = new(2)
        assert fresh.shape == state.shape and fresh.dtype == torch.int32 and not fresh.any()
    else:
        with pytest.raises(RuntimeError, match='no CPU path'):
            reset(state)
        with pytest.raises(RuntimeError, match='no CPU path'):
            new(2)
        assert bool((state == 0x5A5A5A5A).all())


def test_out_planes():
    from mydetection_amd import ops
    dev = torch.device('cpu')
    shapes = {'box': ((2, 3, 5), torch.float32), 'id': ((2, 3), torch.int64), 'count': ((2,), torch.int32)}
    made = ops.out_planes('some_frames', None, shapes, dev)
    assert {k: (tuple(t.shape), t.dtype) for k, t in made.items()} == shapes
    assert all(t.device == dev and t.is_contiguous() for t in made.values())
    back = ops.out_planes('some_frames', made, shapes, dev)
    assert back is made and all(back[k] is made[k] for k in shapes)
    extra = dict(made, other=torch.zeros(1))                         # entries the call does not name are not its business
    assert ops.out_planes('some_frames', extra, shapes, dev) is extra
    wrong = {'box': torch.zeros((2, 3, 4)), 'id': torch.zeros((2, 3), dtype=torch.int32), 'count': torch.zeros((2, 2), dtype=torch.int32)[:, 0]}
    for key, t in wrong.items():
        assert key != 'count' or (tuple(t.shape) == (2,) and not t.is_contiguous())
        with pytest.raises(ValueError, match=rf"some_frames: out\['{key}'\]"):
            ops.out_planes('some_frames', dict(made, **{key: t}), shapes, dev)


def test_classes_rule_of_both_sets():
    from mydetection_amd import ops
    sets = (lambda classes: ops.zone_set(HW, polygons=[[(0, 0), (9, 0), (9, 9)]], classes=classes),
            lambda classes: ops.trail_set(2, classes=classes))
    for make in sets:
        for bad in (list(range(17)), [3, -1], []):
            with pytest.raises(ValueError, match='classes'):
                make(bad)
        s = make([7, 2])
        assert s.n_classes == 2 and list(s.classes[:2]) == [7, 2]
        assert make(None).n_classes == 0
