"""Poisoned arenas for footprint tests (plain torch, runs on any device).

The library's layout contract: a logical [B,C,H,W] tensor is any 16-byte-aligned channel range of a [B,H,W,ld] buffer.  An arena
is ONE flat float32 allocation  [guard | B*H*W*ld | guard]  in which every word starts as a sentinel -- a quiet NaN with a
recognisable payload, compared bit for bit through an int32 view, so a NaN a kernel writes is not mistaken for it.  The view of
channels [c0, c0 + C) goes to the kernel; afterwards the checker says which words outside the view changed, and where.

    out, chk = arena(B, C, H, W, ld, c0, device)              # output arena: the view is poison too
    launch(..., out=out)
    chk.view_defined()                                         # every word of the view was written, and is finite
    chk.outside_untouched()                                    # guards and neighbour channels still hold the fill

    x, chk = arena(B, C, H, W, ld, c0, device, data=values)   # input arena: real data inside, poison around it
"""
import torch

SENTINEL_BITS = 0x7FC0BEEF


def sentinel():
    """The sentinel as a float32 scalar tensor (a NaN: only its bits compare)."""
    return torch.tensor(SENTINEL_BITS, dtype=torch.int32).view(torch.float32)


def guard_floats(W, ld):
    """Guards are a condition, not a measurement: a store that is one image row or one tile off must land inside the arena."""
    return max(W * ld, 4096)


class Checker:
    def __init__(self, flat, guard, B, C, H, W, ld, c0, fill_bits):
        self.flat, self.guard, self.fill_bits = flat, guard, fill_bits
        self.B, self.C, self.H, self.W, self.ld, self.c0 = B, C, H, W, ld, c0

    def _bits(self):
        return self.flat.view(torch.int32)

    def body(self):
        """The [B,H,W,ld] buffer between the guards."""
        n = self.B * self.H * self.W * self.ld
        return self.flat[self.guard:self.guard + n].view(self.B, self.H, self.W, self.ld)

    def view(self):
        return self.body().permute(0, 3, 1, 2)[:, self.c0:self.c0 + self.C]

    def changed_outside(self):
        """(count, [locations]) of the words outside the view that no longer hold the fill value; a location is
        ('guard_lo', offset from the arena's start) | ('guard_hi', offset from the body's end) | ('pixel', b, y, x, channel)."""
        bits = self._bits()
        n = self.B * self.H * self.W * self.ld
        bad = bits != self.fill_bits
        inside = torch.zeros(self.ld, dtype=torch.bool, device=bits.device)
        inside[self.c0:self.c0 + self.C] = True
        body = bad[self.guard:self.guard + n].view(-1, self.ld) & ~inside
        lo, hi = bad[:self.guard], bad[self.guard + n:]
        count = int(lo.sum()) + int(hi.sum()) + int(body.sum())
        where = []
        if count:
            where += [('guard_lo', int(i)) for i in lo.nonzero().flatten()[:4]]
            for pix, ch in body.nonzero()[:8].tolist():
                b, rest = divmod(pix, self.H * self.W)
                y, x = divmod(rest, self.W)
                where.append(('pixel', b, y, x, ch))
            where += [('guard_hi', int(i)) for i in hi.nonzero().flatten()[:4]]
        return count, where

    def outside_untouched(self, what='arena'):
        count, where = self.changed_outside()
        assert count == 0, (f'{what}: {count} word(s) outside the view [B={self.B}, channels {self.c0}..{self.c0 + self.C - 1} of ld '
                            f'{self.ld}, {self.H}x{self.W}] were written; first: {where}')

    def undefined_in_view(self):
        """(count, [(b, y, x, channel)]) of the words of the view that still hold the sentinel."""
        v = self.body().view(torch.int32)[..., self.c0:self.c0 + self.C] == SENTINEL_BITS
        count = int(v.sum())
        where = [(b, y, x, self.c0 + c) for b, y, x, c in v.nonzero()[:8].tolist()] if count else []
        return count, where

    def view_defined(self, what='arena'):
        """A launch must define every word of its view, with finite values."""
        count, where = self.undefined_in_view()
        assert count == 0, f'{what}: {count} word(s) of the view were never written; first (b, y, x, channel): {where}'
        fin = torch.isfinite(self.view())
        assert bool(fin.all()), f'{what}: {int((~fin).sum())} non-finite value(s) in the view'


def arena(B, C, H, W, ld, c0, device, fill='sentinel', data=None):
    """ONE flat float32 buffer [guard | B*H*W*ld | guard], every word `fill` ('sentinel' or 'zero'); returns the logical [B,C,H,W] view
    of channels [c0, c0 + C) (pixel stride ld, 16-byte aligned) and its Checker.  data: values for the view (an input arena);
    without it the view holds the SENTINEL whatever the fill, so that a launch that leaves a word undefined is seen."""
    assert fill in ('sentinel', 'zero') and ld % 4 == 0 and c0 % 4 == 0 and 0 <= c0 and c0 + C <= ld and min(B, C, H, W) >= 1
    guard = (guard_floats(W, ld) + 3) // 4 * 4
    n = B * H * W * ld
    fill_bits = SENTINEL_BITS if fill == 'sentinel' else 0
    flat = torch.full((2 * guard + n,), fill_bits, dtype=torch.int32, device=device).view(torch.float32)
    chk = Checker(flat, guard, B, C, H, W, ld, c0, fill_bits)
    view = chk.view()
    if data is not None:
        assert tuple(data.shape) == (B, C, H, W)
        view.copy_(data)
    else:
        chk.body().view(torch.int32)[..., c0:c0 + C] = SENTINEL_BITS
    assert view.data_ptr() % 16 == 0, 'the allocator returned a buffer that is not 16-byte aligned'
    return view, chk


def flat_arena(n, device, fill='sentinel', data=None):
    """A one-dimensional arena for buffers that are not feature maps (squeeze sums [B,S+1,C], gates [B,C]): the view is `n`
    contiguous floats between two guards.  Expressed as a 1 x n x 1 x 1 map so the same Checker applies."""
    ld = (n + 3) // 4 * 4
    _, chk = arena(1, n, 1, 1, ld, 0, device, fill, None if data is None else data.reshape(1, n, 1, 1))
    return chk.flat[chk.guard:chk.guard + n], chk
