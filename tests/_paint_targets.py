"""What the GPU tests of the kernels that paint into frames share (tests/test_gpu_draw.py, tests/test_gpu_redact.py): the kinds of
target, a target inside a backing buffer whose every byte is compared, and the way arrays go to the device."""
import numpy as np
import torch

KINDS = ('contiguous', 'pitched', 'odd')


class Target:
    """B planes / frames [B, H, W(, C)] of random bytes inside a backing buffer on the device, plus the host copy."""

    def __init__(self, rng, B, H, W, C, kind):
        if kind == 'contiguous':
            pad_y, pad_x, oy, ox, lead = 0, 0, 0, 0, 0
        elif kind == 'pitched':                                       # base, pitch and frame stride multiples of 4; W is not the pitch
            pad_x = 4 + (-(W + 4) * max(C, 1)) % 4
            while ((W + pad_x) * max(C, 1)) % 4:
                pad_x += 1
            pad_y, oy, ox, lead = 0, 0, 0, 0
        else:
            pad_y, pad_x, oy, ox, lead = 5, 7, 2, 3, 1
            if ((W + pad_x) * max(C, 1)) % 2 == 0:
                pad_x += 1                                           # an odd pitch as well
        shape = (B, H + pad_y, W + pad_x) + ((C,) if C else ())
        self.back = rng.integers(0, 256, size=shape, dtype=np.uint8)
        self.lead = rng.integers(0, 256, size=lead, dtype=np.uint8)
        self.flat = torch.from_numpy(np.concatenate([self.lead, self.back.ravel()])).cuda()
        self.view = self.flat[lead:].view(shape)[:, oy:oy + H, ox:ox + W]
        self.host = self.back[:, oy:oy + H, ox:ox + W]               # a view of `back`: the restatement paints into it
        self.n_lead, self.oy, self.ox = lead, oy, ox

    def check(self, what, skip=None):
        """Every byte of the backing buffer equals the host copy (which the restatement painted); skip: bool mask over the
        view [B, H, W] of pixels that are not compared."""
        got = self.flat.cpu().numpy()
        assert np.array_equal(got[:self.n_lead], self.lead), what
        got = got[self.n_lead:].reshape(self.back.shape)
        if skip is not None:
            B, H, W = skip.shape
            region = got[:, self.oy:self.oy + H, self.ox:self.ox + W]
            region[skip] = self.host[skip]
        bad = np.argwhere(got != self.back)
        assert bad.size == 0, (what, len(bad), bad[:5].tolist())


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype=dtype).cuda()
