"""Host-side pieces of the large-tensor tests (tests/_large.py, ops.conv_size_refusals): which images a crossing names, the bounds,
and the launchers' size rules as `ops` restates them for its error messages.  No GPU."""
import torch

from _large import G31, G32, abs_tol, close_tol, crossing_images, image_bytes, rel_tol


def _batch(B, C, H, W, ld=None):
    ld = ld or C
    return torch.empty((B, H, W, ld), dtype=torch.float32, device='meta').permute(0, 3, 1, 2)[:, :C]


def test_crossing_images_name_the_image_that_holds_the_byte():
    x = _batch(1040, 256, 64, 64)                              # 4 MiB / image: byte 2^31 opens image 512, byte 2^32 image 1024
    assert image_bytes(x) == 4 << 20
    assert crossing_images(x) == {511, 512, 513, 1023, 1024, 1025}
    assert crossing_images(_batch(512, 256, 64, 64)) == set()             # exactly 2^31 bytes: no byte 2^31
    assert crossing_images(_batch(513, 256, 64, 64)) == {511, 512}        # ... one image more: the last image holds it
    y = _batch(3650, 144, 32, 64)                              # 1152 KiB / image: the crossings fall INSIDE images 1820 and 3640
    assert G31 // image_bytes(y) == 1820 and G31 % image_bytes(y) != 0
    assert crossing_images(y) == {1819, 1820, 1821, 3639, 3640, 3641}
    padded = _batch(2048, 52, 64, 64, ld=64)                  # a 52-channel view of a 64-wide buffer: the view's pixels span the whole buffer
    assert image_bytes(padded) == 64 * 64 * 64 * 4 and crossing_images(padded) == set() and crossing_images(_batch(2049, 52, 64, 64, ld=64)) == {2047, 2048}
    assert crossing_images(_batch(1100, 240, 64, 64)) == {545, 546, 547, 1091, 1092, 1093} and G32 // (240 * 4096 * 4) == 1092


def test_bounds():
    ref = torch.tensor([[0.5, -4.0]], dtype=torch.float64)
    assert rel_tol(2e-5, True)(ref) == 8e-5 and rel_tol(2e-5, True)(ref * 0.1) == 2e-5 and rel_tol(2e-5, False)(ref * 0.1) == 2e-5 * 0.4
    assert rel_tol(2e-5, True).of_max(4.0) == 8e-5 and abs_tol(1e-5)(ref) == 1e-5 and abs_tol(1e-5).of_max(7.0) == 1e-5
    assert torch.equal(close_tol(1e-5, 1e-4)(ref), 1e-4 + 1e-5 * ref.abs())


def test_conv_size_refusals_restate_the_launchers_rules():
    from mydetection_amd import ops
    L = ops.CONV_OFFSET_LIMIT
    assert L == 0x7FFFFFF0
    # direct implicit GEMM, 1x1 16 -> 64 at 64 x 64: the output passes the limit at batch 2048, not at 2047
    assert ops.conv_size_refusals('igemm', 2047, 64, 64, 64, 64, 16, 64) == []
    (name, nbytes, rule), = ops.conv_size_refusals('igemm', 2048, 64, 64, 64, 64, 16, 64)
    assert (name, nbytes) == ('output', G31) and str(L) in rule
    assert [r[:2] for r in ops.conv_size_refusals('igemm', 2048, 64, 64, 64, 64, 16, 52, 64)] == [('residual', G31)]
    # the batches at which the 640^2 models reach it: a 64-channel 320^2 output at batch 82, a 32-channel 640^2 one at batch 41
    assert ops.conv_size_refusals('igemm', 81, 640, 640, 320, 320, 32, 64) == [] and ops.conv_size_refusals('igemm', 82, 640, 640, 320, 320, 32, 64)
    assert ops.conv_size_refusals('igemm', 40, 640, 640, 640, 640, 32, 32) == [] and ops.conv_size_refusals('igemm', 41, 640, 640, 640, 640, 32, 32)
    # the input window: the images one 256-row tile can touch (2 for maps of more than 256 output pixels)
    assert ops.conv_size_refusals('igemm', 2, 2048, 2048, 1024, 1024, 64, 64)[0][:2] == ('input', 2 * 2048 * 2048 * 64 * 4)
    # Winograd: a window of (tiles / tiles per image + 2) images of the widest of the three tensors, whatever the batch
    assert ops.conv_size_refusals('wino', 8200, 64, 64, 64, 64, 32, 32) == [] and ops.conv_size_refusals('wino4', 4112, 64, 64, 64, 64, 32, 32, 32) == []
    assert [r[0] for r in ops.conv_size_refusals('wino', 1, 2048, 2048, 2048, 2048, 64, 32)] == ['input']
    assert [r[0] for r in ops.conv_size_refusals('wino4', 1, 2048, 2048, 2048, 2048, 32, 32, 64)] == ['residual']
