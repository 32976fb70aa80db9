"""`Bound`: what `Tracker` and the objects that sit behind it in a tracked call (`Zones`, `Overlay`, `CameraMotion`,
`Appearance`) share -- a per-stream state buffer on the device that the first call allocates, and the shape of that call, which
every later call must repeat.  A new per-stream companion is a subclass of this and one state family in ops."""


class Bound:
    """The binding of an object to its first call.  `state`: the int32 [streams, words] device buffer (None before the first
    call, or when the object keeps none), `last`: the output dict of the latest call, `streams`, `max_tracks`, `img_hw`: what
    the first call bound (None before it; max_tracks stays None where the state has no track slots).
    A subclass names itself in `what` (the prefix of the messages) and has two hooks: _allocate(device) makes `state` (and what
    goes with it) on the device from the fields bound just now, _reset_state() puts it back to that.  It may bind one more
    thing: `extra` = (the attribute that holds it, what a message calls it)."""
    what = None
    extra = None
    hint = ''                                                        # closes the message of a call with another shape

    def __init__(self):
        self.state = self.last = None
        self.streams = self.max_tracks = self.img_hw = None

    def _key_text(self, key):
        streams, max_tracks, hw, extra = key
        tracks = '' if max_tracks is None else f'{max_tracks} tracks on '
        more = '' if self.extra is None else f' ({self.extra[1]} {extra!r})'
        return f'{streams} streams of {tracks}{hw[0]}x{hw[1]} frames{more}'

    def _check_bound(self, streams, max_tracks, img_hw, extra=None):
        """The key of a call -- its streams, max_tracks, frame size and the subclass's extra.  A ValueError when the first
        call had another; touches no device."""
        key = (streams, max_tracks, (int(img_hw[0]), int(img_hw[1])), extra)
        if self.img_hw is not None:
            mine = (self.streams, self.max_tracks, tuple(self.img_hw), getattr(self, self.extra[0]) if self.extra else None)
            if key != mine:
                raise ValueError(f'{self.what}: bound to {self._key_text(mine)} by its first call, got {self._key_text(key)}{self.hint}')
        return key

    def _key(self, tracker, img_hw):
        """_check_bound for a call behind `tracker`, as most subclasses bind: its streams and max_tracks and the frame size."""
        return self._check_bound(tracker.streams, tracker.max_tracks, img_hw)

    def bind(self, tracker, img_hw, device):
        """First call: take the tracker's shape and the frame size and allocate on the device.  Returns `state`."""
        return self._bind_key(self._key(tracker, img_hw), device)

    def _bind_key(self, key, device):
        """First call: take the key (_check_bound's) and allocate on the device; an object that keeps no state takes the same
        key again.  Later calls: a ValueError on another device.  Returns `state`."""
        if self.state is None:
            self.streams, self.max_tracks, self.img_hw = key[:3]
            if self.extra:
                setattr(self, self.extra[0], key[3])
            try:
                self._allocate(device)
            except Exception:
                self.img_hw = None                                   # not bound after all: the next call starts over
                raise
        elif self.state.device != device:
            raise ValueError(f'{self.what}: its state lives on {self.state.device}, this call runs on {device}')
        return self.state

    def reset(self):
        """Reset the state, if there is one, and forget `last`.  The binding stays."""
        if self.state is not None:
            self._reset_state()
        self.last = None

    @staticmethod
    def _image_device(image):
        """The device of what a frame source's image() returns first: the frames, or a tuple of planes."""
        return (image[0] if isinstance(image, (tuple, list)) else image).device
