"""GPU tests that run every instance and every branch csrc/motion.hip compiles, each against the restatement
(tests/_motion_ref.py) with == on the shifts, the block rows and every word of the state (tests/test_gpu_motion.py: _run,
_assert_motion_state).  The cases are tables in tests/_motion_cases.py; tests/test_motion_cases_host.py proves without a GPU that
each is what this table takes it for.  The outputs are passed in filled with a pattern, so a word no kernel writes shows.

motion_reduce_kernel, motion_refine_kernel and motion_finish_kernel are instantiated for K in {2, 4, 8} x {RgbLuma, YuvLuma<1,false>
(nv12, nv21), <1,true> (i420), <2,false> (p010), <2,true> (i010)}: motion.hip:446-450, yuv_fetch.h:172-178.  'wide' and 'narrow'
are the memory forms of _device_view below.  mh = csrc/motion.hip, yf = csrc/yuv_fetch.h.

test_every_instance -- every case in one call and in calls of [1, F - 1], whose second takes frame 0's reduced luma and P x P
patches from the state (mh:173-177, mh:361-364)
  instance             case                             branch                                             rule
  <2, RgbLuma>         tests/test_gpu_motion.py         8-byte loads (contiguous); bytes (83x117, crop)    mh:506-507, mh:101-121
  <4, RgbLuma>         rgb-k4-wide                      16-byte loads; bytes in a row's last thread, n < 4 mh:506-507 all % 16 == 0; mh:101, mh:116
                       rgb-k4-narrow                    bytes everywhere                                   mh:507 odd base, odd pitch
  <8, RgbLuma>         rgb-k8-wide, rgb-k8-narrow       as k = 4, six 16-byte loads a row                  mh:108-111
  <2, YuvLuma<1,false>> nv12-k2-wide, nv21-k2-wide      wr = 59: a row's last quad holds 2 samples, read   mh:132 valid - 4 d = 2; yf:47 fails
  <2, YuvLuma<1,true>>  i420-k2-wide                    one by one inside a wide launch                    inside a wide launch -> yf:60-69
  <2, YuvLuma<2,false>> p010-k2-wide                    (k = 2 on planes that allow no wide reads, and
  <2, YuvLuma<2,true>>  i010-k2-wide                    with wr % 4 == 0: tests/test_gpu_motion.py)
  <4, YuvLuma<1,false>> nv12-, nv21-k4-wide / -narrow   wide: 4-byte reads; narrow: samples                yf:151-157 every plane % 4; yf:47-49, yf:60-69
  <4, YuvLuma<1,true>>  i420-k4-wide / -narrow          wide: 4-byte reads; narrow: samples                yf:151-157 Y % 4, U and V % 2
  <4, YuvLuma<2,false>> p010-k4-wide / -narrow          wide: 8-byte reads; narrow: words; yuv_s8          yf:151-157 every plane % 8; yf:52-55, yf:33-40
  <4, YuvLuma<2,true>>  i010-k4-wide / -narrow          wide: 8-byte reads; narrow: words; yuv_s8          yf:151-157 Y % 8, U and V % 4
  <8, YuvLuma<..>> x 4  <layout>-k8-wide / -narrow      as k = 4; two quads a sum: acc[d / (K / 4)]        mh:137
  every k = 8 case: lk2 = 6, P = 32, BW = 8, the 48 x 13-dword refine window, 289 refine candidates       mh:46, mh:51, mh:343-344
  every k = 4, 8 case on planes: wr % 4 != 0, so a row's last thread has n < 4.  valid = n K is a multiple of 4 there: the quads
      beyond it are skipped (mh:131) and none is cut.  Only k = 2 can cut a quad, hence the k = 2 cases above.
  nv12-k4-wide, i010-k4-narrow, p010-k8-wide, i420-k8-narrow: two streams with their own shifts, o = s F + f   mh:251, mh:351, mh:408-409
  p010 / i010 cases: v10 = 4 y + j with j in [-2, 1], up to +3 at y = 255, so the + 2 and the min(255, ..) decide; 1022 and 1023 occur;
      the six ignored bits are random                                                                      yf:37-38
test_medians_of_unequal_block_vectors
  96x128-k2, 160x224-k4    four valid blocks of six, two motions: the lower and the upper median differ in x and in y, coarse
      (fx = 0, mh:333) and final (fx = 4, mh:404), and x and y come from different blocks: m = (n - 1) / 2, mh:308, mh:314.  The
      two flat blocks keep 0, 0 in fields 4 and 5 (mh:281, mh:354), the first frame six zeros a block (mh:255)
test_many_blocks
  272, 1024 (the maximum)  nb > 256: the b += 256 loop of block_median goes round (mh:297), grids of nb workgroups (mh:438, mh:440),
      the stride of the state writer over nb patches (mh:414-423); two motions, so the histograms hold several bins
test_equal_minima
  x, y, diagonal, both     the packed key (mh:228-229) orders equal SADs: dx decides, dy decides, dy before dx decides, the distance
      before both decides
test_odd_search
  R5-k2, R15-k2, R7-k4, R5-k8    16 + 2R is no multiple of 4: another LDS pitch (mh:179, mh:258), a template origin off the dword
      grid (mh:262), sh = cx & 3 against it (mh:185)
test_thresholds_at_equality
  texture_equal, texture_above   smax - smin == min_texture keeps the block, min_texture one higher drops it       mh:285-287
  blocks_equal, blocks_above     n == an explicit min_blocks reports, min_blocks one higher does not               mh:335, mh:466
"""
import numpy as np
import pytest
import torch

import _motion_cases as cases
import _motion_ref as ref
from test_gpu_motion import _run

pytestmark = pytest.mark.gpu

FILL = 0x5a5a5a5a


def _device_view(a, form, rng, held):
    """The host array a [B, h, w, ...] as a device tensor in one of three memory forms:
    packed  contiguous.
    wide    the first w columns of a buffer whose rows hold a multiple of 16 samples (or pixels, or pairs): base, row pitch and
            frame stride are multiples of every wide read.
    narrow  columns 1 .. w of a buffer whose rows hold an odd number of samples: an odd sample offset and an odd pitch.
    The rest of the buffer is random.  held collects (buffer, a copy of it): the estimator reads only."""
    t = torch.from_numpy(a)
    if form == 'packed':
        buf = view = t.cuda()
    else:
        w = a.shape[2]
        wp, x0 = ((w // 16 + 1) * 16, 0) if form == 'wide' else (w + 3 + w % 2, 1)
        shape = a.shape[:2] + (wp,) + a.shape[3:]
        info = np.iinfo(a.dtype)
        buf = torch.from_numpy(rng.integers(info.min, info.max + 1, shape, dtype=a.dtype)).cuda()
        view = buf[:, :, x0:x0 + w]
        view.copy_(t.cuda())
    held.append((buf, buf.clone()))
    return view


def _byte_bits(t):
    """The bits that decide whether wide reads are allowed: address, row pitch and frame stride in bytes, or-ed."""
    return t.data_ptr() | t.stride(0) * t.element_size() | t.stride(1) * t.element_size()


def _device_frames(c, px, held):
    """image_of for _run: frames f0 .. f0 + n - 1 of every stream of px ([S, F, H, W, 3] RGB, or the stored Y plane [S, F, H, W]
    with random chroma planes) in the memory form of the case."""
    rng = np.random.default_rng(5)
    form, source = c['form'], c['source']

    def image_of(f0, n):
        sel = np.array(px[:, f0:f0 + n]).reshape((-1,) + px.shape[2:])
        if source == 'rgb':
            view = _device_view(sel, form, rng, held)
            if form != 'packed':
                assert (_byte_bits(view) % 16 == 0) == (form == 'wide') and (form == 'wide' or _byte_bits(view) % 2)
            return view
        B, H, W = sel.shape
        ch, cw = (H + 1) // 2, (W + 1) // 2
        info = np.iinfo(sel.dtype)
        shapes = [(B, ch, cw)] * 2 if source in ('i420', 'i010') else [(B, ch, cw, 2)]
        planes = [_device_view(p, form, rng, held) for p in [sel] + [rng.integers(info.min, info.max + 1, s, dtype=sel.dtype) for s in shapes]]
        bps = sel.dtype.itemsize
        if form == 'wide':
            assert all(_byte_bits(p) % (4 * bps) == 0 for p in planes)
        else:
            assert _byte_bits(planes[0]) % (4 * bps) and _byte_bits(planes[0]) % bps == 0
        return planes

    return image_of


def _check(group, name, splits=None):
    c = cases.case(group, name)
    px, _ = cases.scene(group, name)
    _, shift, blocks, streams = cases.want(group, name)
    held = []
    _run(_device_frames(c, px, held), None, c['hw'], px.shape[0], splits=splits, layout=None if c['source'] == 'rgb' else c['source'],
         want=(shift, blocks, streams), fill=FILL, **c['set'])
    assert held and all(torch.equal(buf, keep) for buf, keep in held)                     # read only


@pytest.mark.parametrize('name', sorted(cases.INSTANCES))
def test_every_instance(name):
    """One call, and calls of [1, F - 1] whose second takes frame 0's predecessor from the state."""
    c = cases.INSTANCES[name]
    if c['source'] in ('p010', 'i010'):
        v10 = ref.live_bits(cases.scene('instance', name)[0], c['source'])
        assert (v10 == 1022).any() and (v10 == 1023).any()
    F = len(c['shifts'][0]) + 1
    _check('instance', name)
    _check('instance', name, splits=[1, F - 1])


@pytest.mark.parametrize('name', sorted(cases.MEDIANS))
def test_medians_of_unequal_block_vectors(name):
    """Four valid blocks of six with two motions: an upper median, an off-by-one bin or x and y taken from one block would show.
    The outputs start as FILL: the two flat blocks still read 0, 0 in fields 4 and 5, the first frame six zeros a block."""
    _, _, blocks, _ = cases.want('medians', name)
    assert not blocks[0, 0].any() and not blocks[0, 1, [2, 5], 4:].any() and blocks[0, 1, [0, 1, 3, 4], 4:].any(axis=1).all()
    _check('medians', name)


@pytest.mark.parametrize('name', sorted(cases.MANY))
def test_many_blocks(name):
    _check('many', name)


@pytest.mark.parametrize('name', sorted(cases.PERIODIC))
def test_equal_minima(name):
    _check('periodic', name)


@pytest.mark.parametrize('name', sorted(cases.ODD))
def test_odd_search(name):
    _check('odd', name)
    _check('odd', name, splits=[2, 2])


@pytest.mark.parametrize('name', cases.THRESHOLDS)
def test_thresholds_at_equality(name):
    _check('threshold', name)
