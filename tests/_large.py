"""The helper of tests/test_gpu_large_tensors.py: one `ops` call on a batch whose tensors pass 2^31 and 2^32 bytes.

run_large(dev, what, call, batched, tols, ref64, ...) does, for a call whose tensors are batch-major:

  * whole run: `call(**batched)` once on the whole batch, under an ops.KernelTimer; the span of the intended kernel must be the only
    one recorded;
  * differential check, every image: the same call on batch chunks -- views t[b0:b1] of the same storage, every tensor of a chunk
    below 1 GiB, a fresh chunk-sized output -- against the matching slice of the whole run, on the device: bit-identical
    (`exact=True`: the launcher's plan does not depend on B) or within twice the output's float64 tolerance (both runs are within
    one tolerance of the truth);
  * float64 check, named images: images 0 and B - 1, and for every tensor of the call and each of 2^31 and 2^32 that its byte size
    exceeds, the image that holds that byte and its two neighbours (plus `extra_named`: crossings in a workspace).  The reference is
    computed on the CPU in float64 from those images alone.

Inputs are made on the device by a seeded device generator (`randn_nhwc` / `rand_nchw`): every image is different, so a read from
the wrong image is visible in both checks.  Returns the measured peak of live device memory and the wall time, and asserts the peak
stays under 24 GiB.
"""
import time

import torch

G31, G32 = 1 << 31, 1 << 32
CHUNK_BYTES = 1 << 30
MEMORY_LIMIT = 24 << 30


def randn_nhwc(gen, B, C, H, W, ld=None, c0=0):
    """A logical [B,C,H,W] view of a fresh [B,H,W,ld] normal buffer (channels [c0, c0 + C)), made on the generator's device."""
    ld = ld or (C + 3) // 4 * 4
    buf = torch.empty((B, H, W, ld), dtype=torch.float32, device=gen.device)
    buf.normal_(generator=gen)
    return buf.permute(0, 3, 1, 2)[:, c0:c0 + C]


def rand_nchw(gen, B, C, H, W, lo=0.0, hi=1.0):
    """A contiguous [B,C,H,W] uniform image batch in [lo, hi)."""
    x = torch.empty((B, C, H, W), dtype=torch.float32, device=gen.device)
    x.uniform_(lo, hi, generator=gen)
    return x


def image_bytes(t):
    return t.stride(0) * t.element_size()


def crossing_images(t):
    """Images of a batch-major tensor that hold byte 2^31 / 2^32 of it, with their neighbours."""
    s, B = image_bytes(t), t.shape[0]
    named = set()
    for beta in (G31, G32):
        if s * B > beta:
            i = beta // s
            named |= {i - 1, i, i + 1}
    return {i for i in named if 0 <= i < B}


def rel_tol(rel, floor1=True):
    """The conv families' bound (tests/test_gpu_footprint.py FAMILY_TOL): rel * max|ref| (at least rel when floor1)."""
    def bound(ref):
        return bound.of_max(ref.abs().max().item())
    bound.of_max = lambda m: rel * (max(1.0, m) if floor1 else m)
    return bound


def abs_tol(a):
    bound = lambda ref: a                                   # noqa: E731
    bound.of_max = lambda m: a
    return bound


def close_tol(rtol, atol):
    """numpy.testing.assert_allclose's bound, elementwise."""
    return lambda ref: atol + rtol * ref.abs()


EXACT = abs_tol(0.0)


def _tuple(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v,)


def _worst(diff, bound):
    """max(diff - bound) <= 0 for a scalar or elementwise bound; returns (largest diff, bound there)."""
    if torch.is_tensor(bound):
        over = diff - bound
        i = int(over.argmax())
        return diff.flatten()[i].item(), bound.flatten()[i].item()
    return diff.max().item(), bound


def run_large(dev, what, call, batched, tols, ref64, *, span, exact, reduce=None, extra_named=(), crossing=True):
    """call(**batched) -> one output or a tuple of batch-major outputs; tols: one bound maker per output (rel_tol / abs_tol /
    close_tol / EXACT); crossing=False: a guard's accepted side, whose tensors stay just below 2^31 bytes; ref64(**cpu_float64_images) -> the float64 reference(s) of those images; reduce: per output None or a function
    applied to the kernel's output before it meets the reference (e.g. per-slice sums -> per-image sums)."""
    from mydetection_amd import ops
    B = next(iter(batched.values())).shape[0]
    assert all(t.shape[0] == B for t in batched.values())
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()

    def timed(**kw):
        ops.TIMER = ops.KernelTimer()
        try:
            out = _tuple(call(**kw))
        finally:
            timer, ops.TIMER = ops.TIMER, None
        if span is not None:
            assert set(timer.spans) == {span}, f'{what}: launches {sorted(timer.spans)}, expected only {span}'
        return out

    whole = timed(**batched)
    assert len(whole) == len(tols) and all(o.shape[0] == B for o in whole)
    reduce = reduce or [None] * len(whole)
    crossed = {name: sorted(crossing_images(t)) for name, t in list(batched.items()) + [(f'output {k}', o) for k, o in enumerate(whole)]}
    assert any(crossed.values()) or not crossing, f'{what}: no tensor passes 2^31 bytes'

    # ---- float64, named images
    named = sorted({0, B - 1} | {i for v in crossed.values() for i in v} | {i for i in extra_named if 0 <= i < B})
    idx = torch.tensor(named, device=dev)
    refs = _tuple(ref64(**{k: v[idx].cpu().double() for k, v in batched.items()}))
    assert len(refs) == len(whole)
    report = []
    for k, (o, ref, tol, red) in enumerate(zip(whole, refs, tols, reduce)):
        got = o[idx].cpu().double()
        got = red(got) if red else got
        assert got.shape == ref.shape, (what, k, tuple(got.shape), tuple(ref.shape))
        assert bool(torch.isfinite(got).all()), f'{what}: output {k} has non-finite values in images {named}'
        bound = tol(ref)
        diff = (got - ref).abs()
        err, at = _worst(diff, bound)
        per_image = diff.flatten(1).max(dim=1).values
        report.append(f'output {k}: float64 err {err:.3e} (bound {at:.3e}) on images {named}')
        assert err <= at, (f'{what}: output {k} misses float64 by {err:.3e} > {at:.3e}; worst image {named[int(per_image.argmax())]} of {named}, '
                           f'crossings {crossed}')

    # ---- every image: chunks of the same storage against the whole run
    tensors = list(batched.values()) + list(whole)
    n = min((CHUNK_BYTES - 1) // image_bytes(t) for t in tensors)
    assert n >= 2
    n = -(-B // -(-B // n))                             # equal chunks: no small last one that a launcher's size rule would route elsewhere
    # (max|y| of the whole run without a temporary of its size)
    scale = [None if exact else 2.0 * tol.of_max(max(o.max().item(), -o.min().item())) for o, tol in zip(whole, tols)]
    worst = [0.0] * len(whole)
    for b0 in range(0, B, n):
        b1 = min(B, b0 + n)
        if b1 - b0 < 2 and b0 > 0:                      # (a one-image view has no batch stride to check: take the last two)
            b0 = b1 - 2
        part = timed(**{k: v[b0:b1] for k, v in batched.items()})
        for k, (o, p) in enumerate(zip(whole, part)):
            w = o[b0:b1]
            assert p.shape == w.shape
            if exact:
                assert torch.equal(p, w), (f'{what}: output {k} of images [{b0}, {b1}) differs between the whole batch and the chunk in '
                                           f'{int((p != w).sum())} value(s); first image {b0 + int((p != w).flatten(1).any(1).nonzero()[0])}')
            else:
                d = (p - w).abs().flatten(1).max(dim=1).values
                worst[k] = max(worst[k], d.max().item())
                bound = scale[k]
                assert worst[k] <= bound, (f'{what}: output {k}, image {b0 + int(d.argmax())}: whole batch and chunk differ by {worst[k]:.3e} > '
                                           f'{bound:.3e} (twice the float64 tolerance)')
        del part
    torch.cuda.synchronize()
    secs = time.perf_counter() - t0
    peak = torch.cuda.max_memory_allocated()
    sizes = ', '.join(f'{name} {image_bytes(t) * B / 2 ** 20:.0f} MiB' for name, t in list(batched.items()) + [(f'y{k}', o) for k, o in enumerate(whole)])
    print(f'LARGE {what}: B {B}, {sizes}; chunks of {n}; ' + '; '.join(report) +
          ('' if exact else f'; chunk-vs-whole max diff {worst}') + f'; peak {peak / 2 ** 30:.2f} GiB, {secs:.1f} s')
    assert peak < MEMORY_LIMIT, f'{what}: peak device memory {peak / 2 ** 30:.1f} GiB'
    return whole
