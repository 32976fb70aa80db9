"""Torch-tensor front end of the C ABI (include/mydet.h).

PyTorch is plumbing here: tensors are HBM allocations plus the current HIP stream.
Activations are logical NCHW tensors stored channels-last (physical [B,H,W,ld]) so
module inputs/outputs have the reference's shapes while kernels see NHWC.
Every function launches hand-written HIP kernels; no arithmetic falls back to ATen (a
input in a foreign layout is re-laid out with one tensor copy before the launch).
"""
import collections
import ctypes
import functools
import math
import os
import threading

import numpy as np
import torch

from . import _lib

ACT_NONE, ACT_LEAKY, ACT_SWISH = 0, 1, 2
DECODE_YOLO, DECODE_RETINA, DECODE_FCOS, DECODE_RAPID = 0, 1, 2, 3
TOPK = 512


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class KernelTimer:
    """Optional per-launch timing with HIP events recorded on the launch stream (bench.py uses it to
    price the dominant kernel inside the timed region).  Disabled (None) by default: zero overhead."""

    def __init__(self, chain=False):
        self.spans = {}
        self.bytes = {}                  # name -> algorithmic bytes (operands read once + result written once)
        # name -> bytes a maximally fused implementation would still move: tensors that exist only between two layers of a
        # block the reference itself treats as a unit (the 6x-wide maps inside an MBConv block, the depthwise result
        # inside a separable conv) are not counted; block inputs / outputs, weights and residuals are
        self.fused = {}
        # chain=True: the event that closes one launch also opens the next one (every launch of the step is timed and
        # they run back to back on one in-order stream, so "end of launch i" IS "start of launch i+1"): half the
        # event records -- each is a small packet on the GPU's queue -- inside the timed region
        self.chain = chain
        self._tail = None

    def start(self):
        if self.chain and self._tail is not None:
            return self._tail
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()                      # torch's current stream == the stream handed to the C ABI
        return ev

    def stop(self, name, start_ev, work=0.0, nbytes=0.0, fused=None):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        self._tail = ev
        self.spans.setdefault(name, []).append((start_ev, ev, work))
        self.bytes[name] = self.bytes.get(name, 0.0) + nbytes
        self.fused[name] = self.fused.get(name, 0.0) + (nbytes if fused is None else fused)

    def cut(self):
        """Forget the chain (call where untimed GPU work, a synchronisation or a step boundary intervenes)."""
        self._tail = None

    def summary(self):
        """name -> (launches, total_ms, total_work); call after torch.cuda.synchronize()."""
        return {k: (len(v), sum(a.elapsed_time(b) for a, b, _ in v), sum(w for _, _, w in v))
                for k, v in self.spans.items()}


TIMER = None        # set to a KernelTimer() to record
TIMER_DETAIL = False  # name conv launches by shape (tools/profile_layers.py)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def require_gpu(t, what):
    if not t.is_cuda:
        raise RuntimeError(f'{what}: tensor is on {t.device}; mydetection_amd runs on MI355X only '
                           '(there is no CPU path in this package)')


def nhwc_ld(x):
    """Pixel stride of a logical [B,C,H,W] tensor stored as [B,H,W,ld], or None if it is not."""
    B, C, H, W = x.shape
    sb, sc, sh, sw = x.stride()
    if x.dtype != torch.float32 or (C > 1 and sc != 1):
        return None
    ld = sw if W > 1 else (sh if H > 1 else (sb if B > 1 else C))
    if ld < C or ld % 4 or (W > 1 and sw != ld) or (H > 1 and sh != W * ld) or (B > 1 and sb != H * W * ld):
        return None
    if x.data_ptr() % 16:
        return None
    return ld


def to_nhwc(x):
    """Return (tensor, ld) with the tensor in a kernel-readable channels-last layout."""
    ld = nhwc_ld(x)
    if ld is not None:
        return x, ld
    B, C, H, W = x.shape
    Cp = (C + 3) // 4 * 4
    buf = x.new_zeros((B, H, W, Cp)) if Cp != C else x.new_empty((B, H, W, Cp))
    buf[..., :C] = x.permute(0, 2, 3, 1)
    return buf.permute(0, 3, 1, 2)[:, :C], Cp


def empty_nhwc(B, C, H, W, device, ld=None):
    ld = ld or (C + 3) // 4 * 4
    buf = torch.empty((B, H, W, ld), dtype=torch.float32, device=device)
    return buf.permute(0, 3, 1, 2)[:, :C], ld


_WORKSPACE = {}
WORKSPACE_BYTES = 64 << 20
_LANE = 0


class lane:
    """`with ops.lane(i):` -- launches issued inside use lane i's scratch buffers.  Scratch is reused in stream order,
    so two launch sequences that run on different streams at the same time (graph.GraphedPath's batch lanes) must not
    share it; everything outside a `with` is lane 0."""
    def __init__(self, index):
        self.index = int(index)

    def __enter__(self):
        global _LANE
        self.prev, _LANE = _LANE, self.index

    def __exit__(self, *exc):
        global _LANE
        _LANE = self.prev


def _scratch_key(device):
    """(device, lane, host thread): scratch buffers are reused in stream order by ONE launch sequence, so a second host thread that
    happens to be on the same lane index gets buffers of its own.  Not keyed by stream: a hipGraph is warmed
    up on one stream and captured on another, and must find the buffers its warm-up sized (growth during capture raises)."""
    return (device.type, device.index, _LANE, threading.get_ident())


def conv_workspace(device):
    """Per-device, per-lane, per-stream scratch for the split-K tail of conv2d (stream-ordered reuse)."""
    key = _scratch_key(device)
    if key not in _WORKSPACE:
        _WORKSPACE[key] = torch.empty(WORKSPACE_BYTES // 4, dtype=torch.float32, device=device)
    return _WORKSPACE[key]


_WINO4_WS = {}


def wino4_workspace(device, nbytes):
    """Per-device, per-lane scratch for the transform-domain input of the F(4x4,3x3) kernel: grows to the largest layer
    seen (stream-ordered reuse; one stream per lane).  A hipGraph must be captured after an eager pass has sized it.
    Growth REPLACES the buffer: whoever recorded its address (a captured hipGraph) keeps the superseded tensor alive
    through `live_workspaces` -- graph.GraphedPath does -- so a replay never writes into memory the caching allocator
    has handed to someone else."""
    key = _scratch_key(device)
    ws = _WINO4_WS.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        if device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('wino4_workspace: the workspace would grow during stream capture; run the model once eagerly first')
        ws = _WINO4_WS[key] = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)
    return ws


_SE_SHARES = {}
SE_MAX_CSE = 96
# MYDET_SE_IN_DW=0: the squeeze-excite gate as a launch of its own (mydet_se_gate_f32) behind every depthwise launch (A/B)
SE_IN_DW = os.environ.get('MYDET_SE_IN_DW', '1') != '0'
# The in-launch tail is used from this many (expanded) channels up.  Measured per block on a lane of 8 images
# (profiles/r05_se_in_dw.txt: depthwise + gate launch vs depthwise launch with the tail): 1152 channels 34.5 -> 25.3 us,
# 1920 channels 48.0 -> 36.6 us -- the gate launch is a 13-32 us chain of dependent round trips on one CU per image there --,
# but +-1 us at 16 .. 672 channels (the gate launch costs 7-10 us, the finishing workgroup about as much) and 3 us WORSE in
# the fused expand + depthwise launches, so the narrow blocks keep the separate launch.  MYDET_SE_IN_DW_MIN_C overrides.
SE_IN_DW_MIN_C = int(os.environ.get('MYDET_SE_IN_DW_MIN_C', '1000'))


def se_shares(device, n_pairs):
    """Per-device, per-lane share buffer of the in-launch squeeze-excite tail (include/mydet.h: mydet_se_tail.hpart): a header
    (launch counter = 1, finished-image count = 0) followed by room for `n_pairs` (value, epoch) pairs (0).  The kernels' own protocol keeps it consistent, so
    ONE buffer serves every layer of a lane's stream.  Grows to the largest layer seen (not during a stream capture)."""
    key = _scratch_key(device)
    buf = _SE_SHARES.get(key)
    need = _lib.SE_EPOCH_WORDS + 2 * int(n_pairs)
    if buf is None or buf.numel() < need:
        if device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('se_shares: the share buffer would grow during stream capture; run the model once eagerly first')
        buf = torch.zeros(max(need, 1 << 21), dtype=torch.int32, device=device)
        buf[0] = 1                                           # the launch counter; word 1 = images finished in a running launch
        _SE_SHARES[key] = buf = buf.view(torch.float32)
    return buf


def se_tail_timeouts(device):
    """Number of in-launch squeeze-excite tails (summed over this thread's lanes' share buffers) whose finishing workgroup gave up
    waiting for a share and wrote a NaN gate (header word 2 of the share buffer, csrc/se_tail.h): 0 unless a launch was starved
    for ~2^14 polls.  Synchronises."""
    n = 0
    for k, buf in _SE_SHARES.items():
        if k[:2] == (device.type, device.index):
            n += int(buf.view(torch.int32)[2].item())
    return n


def _se_tail(se, B, C, groups, device):
    """(ctypes struct, gate tensor, tensors to keep alive) for `se` = (w1 [Cse,C], b1, w2t [Cse,C], b2) or (None, None, ())."""
    if se is None:
        return None, None, ()
    w1, b1, w2t, b2 = se
    Cse = w1.shape[0]
    assert tuple(w1.shape) == (Cse, C) and tuple(w2t.shape) == (Cse, C) and w1.is_contiguous() and w2t.is_contiguous()
    assert Cse <= SE_MAX_CSE and groups > 0
    gate = torch.empty((B, C), dtype=torch.float32, device=device)
    hpart = se_shares(device, B * groups * Cse)
    t = _lib.SeTail(w1.data_ptr(), b1.data_ptr(), w2t.data_ptr(), b2.data_ptr(), gate.data_ptr(), hpart.data_ptr(), Cse, hpart.numel() * 4)
    return t, gate, (hpart, w1, b1, w2t, b2)


def live_workspaces(device):
    """The scratch tensors launches on `device` are currently handed (split-K workspace, F(4x4) transform-domain
    input).  A captured launch sequence holds on to this list for as long as it can be replayed."""
    key = (device.type, device.index)
    return [t for d in (_WORKSPACE, _WINO4_WS, _SE_SHARES) for k, t in d.items() if k[:2] == key]


def conv_out_size(n, k, stride, pad_lo, pad_hi):
    return (n + pad_lo + pad_hi - k) // stride + 1


# MYDET_CONV_WINO=0 keeps every 3x3 layer on the direct implicit-GEMM kernel (A/B measurements)
WINOGRAD = os.environ.get('MYDET_CONV_WINO', '1') != '0'


def wino_weights(w_ohwi):
    """Transform-domain copy of a 3x3 OHWI weight for `conv2d(..., wino=)`, or None when the shape is not covered
    (Cin % 8, Cout % 4) -- the layer then stays on the direct kernel."""
    require_gpu(w_ohwi, 'wino_weights')
    Cout, kh, kw, Cin = w_ohwi.shape
    if kh != 3 or kw != 3 or Cout % 4:
        return None
    n = _lib.lib().mydet_wino_weights_floats(Cout, Cin)
    if n <= 0:
        return None
    u = torch.empty(n, dtype=torch.float32, device=w_ohwi.device)
    w = w_ohwi.contiguous()
    _lib.check(_lib.lib().mydet_wino_weights_f32(_ptr(w), Cout, Cin, _ptr(u), _stream()), 'mydet_wino_weights_f32')
    return u


# F(4x4,3x3) for the 3x3 layers with Cin >= WINO4_MIN_CIN whose grid fills the chip (>= WINO4_MIN_ITEMS workgroups of
# 32 tiles x 32 channels; smaller grids stay on F(2x2,3x3), which cuts them along K); MYDET_CONV_WINO4=0 turns it off.
# 512 = one full round of the resident workgroups (round 4; 768 before): the 16^2 layers of batch 32 at 512^2 are exactly
# that (2 134 -> 2 289 images/s), the FCOS head's dense 3x3 at 80^2 in a 16-image lane has 600 (+0.5 %)
WINOGRAD4 = os.environ.get('MYDET_CONV_WINO4', '1') != '0'
WINO4_MIN_CIN = int(os.environ.get('MYDET_WINO4_MIN_CIN', '64'))
WINO4_MIN_ITEMS = int(os.environ.get('MYDET_WINO4_MIN_ITEMS', '512'))


def wino4_items(B, H, W, Cout):
    """Workgroups of the F(4x4,3x3) kernel for one layer: 32 tiles of 4x4 outputs x 32 output channels each."""
    return -(-(B * -(-H // 4) * -(-W // 4)) // 32) * -(-Cout // 32)


def wino4_weights(w_ohwi):
    """Transform-domain copy of a 3x3 OHWI weight for the F(4x4,3x3) kernel (`conv2d(..., wino4=)`), or None when the
    shape is not covered (Cin % 4, Cout % 4)."""
    require_gpu(w_ohwi, 'wino4_weights')
    Cout, kh, kw, Cin = w_ohwi.shape
    if kh != 3 or kw != 3 or Cout % 4:
        return None
    n = _lib.lib().mydet_wino4_weights_floats(Cout, Cin)
    if n <= 0:
        return None
    u = torch.empty(n, dtype=torch.float32, device=w_ohwi.device)
    w = w_ohwi.contiguous()
    _lib.check(_lib.lib().mydet_wino4_weights_f32(_ptr(w), Cout, Cin, _ptr(u), _stream()), 'mydet_wino4_weights_f32')
    return u


# MYDET_CONV_SPLIT_BF16=0 keeps every direct conv on the float32 matrix instruction (A/B measurements)
SPLIT_BF16 = os.environ.get('MYDET_CONV_SPLIT_BF16', '1') != '0'


# The split-bf16 form takes a direct-conv layer from this many output pixels (B * Ho * Wo) up -- below, the float32 kernel's
# small-grid K cut is the tuned path (batch-1 layers) -- and, for 1x1 layers, from 128 output channels (tools/r05_b3.py:
# 128->64 @160^2 0.197 vs 0.187 ms for the float32 kernel; every wider shape of the headline 1.25-1.35 x faster)
B3_MIN_ROWS = int(os.environ.get('MYDET_B3_MIN_ROWS', '8192'))
B3_MIN_FLOP = float(os.environ.get('MYDET_B3_MIN_FLOP', '3e9'))
B3_KPAD = os.environ.get('MYDET_B3_KPAD', '1') != '0'      # 1x1 layers with Cin % 16 == 4, 8, 12 (last slab zero-filled)
# The EfficientNet expand convs (1x1, 6 x Cin output channels, swish) take it from fewer rows: on a batch lane of 8 / 16 images
# the 20^2 layers have 3 200 / 6 400 rows and still fill the chip (225-750 tiles of 128 x 128).  Measured in the model, two
# lanes (tools/r05_b3_effnet.sh, two runs each): expand convs on the float32 instruction 3 721 / 4 211 images/s (D1 batch 16 /
# D1-FCOS batch 32), split-bf16 from 8 192 rows 3 761 / 4 268, from 3 000 rows 3 859 / 4 350.  MYDET_B3_EXPAND_MIN_ROWS=0 = off.
B3_EXPAND_MIN_ROWS = int(os.environ.get('MYDET_B3_EXPAND_MIN_ROWS', '3000'))
# ... and the gated project convs (1x1, no activation, the squeeze-excite gate applied to the activations before they are split) from 64
# output channels and the same 3 000 rows.  Their grids are small (80-320 output channels: 50-200 tiles of 128 x 128 on a lane), so the
# launcher cuts a layer of at most cus / 2 such tiles into 64-row tiles.  Measured (tools/r05_b3_gate.sh, tools/r05_b3_half.sh; two to four
# runs each, one call): D1 batch 16 3 854 -> 3 893, D1-FCOS batch 32 4 407 -> 4 500 images/s; with 128-row tiles only, D1 LOST 1-2 %
# (3 851 -> 3 782) while D1-FCOS gained 1 %.  MYDET_B3_GATED_MIN_COUT=0 keeps them all on the float32 kernel.
B3_GATED_MIN_COUT = int(os.environ.get('MYDET_B3_GATED_MIN_COUT', '64'))
B3_GATED_MIN_ROWS = int(os.environ.get('MYDET_B3_GATED_MIN_ROWS', '3000'))


def b3_takes(M, Cin, Cout, k, min_rows=None, min_cout=128):
    """True when `conv2d(..., b3=)` runs the split-bf16 kernel for a layer of this shape."""
    if not SPLIT_BF16 or not (k > 1 or Cout >= min_cout):
        return False
    if Cin % 16 and not (B3_KPAD and k == 1 and Cin % 4 == 0):           # a 16-channel slab never straddles taps; a 1x1 layer's last slab may be short
        return False
    if min_rows is not None:
        return M >= min_rows
    # ... and from 3 GFLOP per launch: below, the float32 kernel's small tiles and K cut are the tuned path.  Batch 1 at 512^2 has two
    # layers past the row limit (32->64 and 64->128 stride 2: 2.4 GFLOP each on 512 / 128 tiles): 1.560 ms per image with them on
    # this kernel, 1.427 without (two runs each in one call); the smallest layers that gain at batch 32 have 3.4 GFLOP.
    return M >= B3_MIN_ROWS and 2.0 * M * k * k * Cin * Cout >= B3_MIN_FLOP


B3Plan = collections.namedtuple('B3Plan', 'form bm bn wn main tail cuts')
B3_FORM_DEFAULT, B3_FORM_WIDE, B3_FORM_WAVES8 = 0, 1, 2


def b3_plan(B, Ho, Wo, Cin, Cout, taps, gated=False, workspace_bytes=None, cus=256):
    """The launch plan of mydet_conv2d_igemm_b3_f32 for a layer on a chip of `cus` CUs (mydet_conv_b3_plan: the launcher's own function,
    host only, under the MYDET_B3_* switches as last read): tile form, BM x BN tile, waves along N, workgroups of the main launch,
    tail tiles cut along K and cuts per tail tile (0 / 1: no tail).  A negative MYDET_E_* code for a shape the entry point refuses."""
    out = (ctypes.c_int32 * 7)()
    ws = WORKSPACE_BYTES if workspace_bytes is None else workspace_bytes
    code = _lib.lib().mydet_conv_b3_plan(B, Ho, Wo, Cin, Cout, taps, int(bool(gated)), ws, cus, out)
    return code if code else B3Plan(*out)


# conv_p3_kernel (csrc/conv_p3.hip: 3x3 conv with the workgroup's input patch resident in LDS, split-bf16 operands) takes a 3x3 pad-1
# layer when its 128-pixel tiles are mostly real pixels (P3_MIN_FILL; ragged 8 x 16 tiles waste their rows -- without strip tiles
# 256->512 @80->40 ran 0.65 vs 0.61 ms, 512->1024 @40->20 0.92 vs 0.69), the launch fills the chip (P3_MIN_WGS workgroups) and
#   stride 2: always (the first three stride-2 layers of Darknet-53 at 640^2: 1.07-1.11 x over conv_igemm_b3_kernel);
#   stride 1: only below WINO4_MIN_CIN input channels, where F(4x4) does not go (32->64 @320^2: 1.16-1.18 x over F(2x2)).
# profiles/r06_conv_p3.txt.  MYDET_CONV_P3=0 turns it off.
CONV_P3 = os.environ.get('MYDET_CONV_P3', '1') != '0'
P3_MIN_WGS = int(os.environ.get('MYDET_P3_MIN_WGS', '512'))             # a full round of the chip (two workgroups per CU); 512^2 batch 32: the 256->512
                                                                        # stride-2 layer @64->32 (1 024 workgroups) joins: 2 601-2 622 vs 2 597-2 601 images/s
P3_S1_MAX_CIN = int(os.environ.get('MYDET_P3_S1_MAX_CIN', '32'))      # stride-1 layers up to this many input channels
# tiles must be mostly real pixels: 0.75 admits the 40-wide (13 tiles for 1 600 pixels: 0.96) and 20-wide (4 for 400: 0.78) maps of Darknet-53 at
# 640^2 with their strip tiles, not a ragged 8 x 16 column on a 20-wide map (0.52)
P3_MIN_FILL = float(os.environ.get('MYDET_P3_MIN_FILL', '0.75'))

P3Plan = collections.namedtuple('P3Plan', 'bn strip tx_n ty_n main_tiles tiles_img ntn lds')


@functools.lru_cache(maxsize=None)
def p3_plan(Ho, Wo, Cout, stride):
    """The tile plan mydet_conv3x3_p3_f32 launches for an Ho x Wo x Cout output map (mydet_conv3x3_p3_plan: the launcher's own function,
    csrc/conv_p3.hip, MYDET_P3_FORM / MYDET_P3_STRIP included): 8 x 16 tiles; at stride 2 a remainder of 8 / 4 columns goes to 16 x 8 /
    32 x 4 strip tiles (strip 1 / 2), any other remainder to a ragged column.  Memoised: the eager conv2d path asks per layer and call."""
    out = (ctypes.c_int32 * 8)()
    _lib.check(_lib.lib().mydet_conv3x3_p3_plan(Ho, Wo, Cout, stride, out), 'mydet_conv3x3_p3_plan')
    return P3Plan(*out)


def p3_tiles(Ho, Wo, stride):
    """Workgroup tiles of 128 output pixels per image and channel tile that mydet_conv3x3_p3_f32 launches."""
    return p3_plan(Ho, Wo, 64, stride).tiles_img


def p3_takes(B, Ho, Wo, Cin, Cout, k, stride, pad):
    """True when conv2d(..., b3=) hands the layer to conv3x3_p3."""
    if not (CONV_P3 and SPLIT_BF16) or k != 3 or stride not in (1, 2) or tuple(pad) != (1, 1, 1, 1) or Cin % 16:
        return False
    plan = p3_plan(Ho, Wo, Cout, stride)
    if B * plan.tiles_img * plan.ntn < P3_MIN_WGS or Ho * Wo < P3_MIN_FILL * 128 * plan.tiles_img:
        return False
    return stride == 2 or Cin <= P3_S1_MAX_CIN


def split_bf16(w_ohwi):
    """The weight operand of `conv2d(..., b3=)`: the OHWI weight [Cout, kh, kw, Cin] as three bfloat16 planes, w = p0 + p1 + p2 to
    2^-27 |w|, in the split-bf16 kernels' slab-major order (include/mydet.h: mydet_split_bf16_f32); int16 storage.
    None when Cin % 16 (a 1x1 weight: when Cin % 4; its last 16-channel slab is zero-filled)."""
    require_gpu(w_ohwi, 'split_bf16')
    Cout = w_ohwi.shape[0]
    K = w_ohwi.numel() // Cout
    n = _lib.lib().mydet_split_bf16_elems(Cout, K)
    one_tap = w_ohwi.shape[1] == 1 and w_ohwi.shape[2] == 1
    if n <= 0 or (w_ohwi.shape[-1] % 16 and not (one_tap and w_ohwi.shape[-1] % 4 == 0)):
        return None
    w = w_ohwi.contiguous().float()
    out = torch.empty(n, dtype=torch.int16, device=w.device)
    _lib.check(_lib.lib().mydet_split_bf16_f32(_ptr(w), Cout, K, _ptr(out), _stream()), 'mydet_split_bf16_f32')
    return out


# The conv kernels address their tensors through buffer descriptors with 32-bit byte offsets (csrc/common.h: mydet_rsrc covers at
# most this many bytes, 16 short of 2 GiB); each launcher refuses (MYDET_E_UNSUPP) what its offsets cannot reach -- INTEGRATION.md,
# "Limits the reference does not have"
CONV_OFFSET_LIMIT = 0x7FFFFFF0


def conv_size_refusals(family, B, H, W, Ho, Wo, ldx, ldy, ldr=0):
    """The size rules of one conv launcher that a layer breaks: [(tensor, bytes, rule)], empty when its size is not the reason of a
    refusal.  family: 'igemm' (mydet_conv2d_igemm_f32 / _b3_f32: the whole output and residual, and the input images one 256-row tile
    can touch), 'wino' / 'wino4' (mydet_conv2d_wino_f32 / _wino4_f32: the images of any of the three tensors that one workgroup's
    64 / 32 tiles can touch).  ldr = 0: no residual."""
    out = []
    if family == 'igemm':
        for name, ld in (('output', ldy), ('residual', ldr)):
            if B * Ho * Wo * ld * 4 >= CONV_OFFSET_LIMIT:
                out.append((name, B * Ho * Wo * ld * 4, f'the whole {name} of the direct implicit GEMM must stay below {CONV_OFFSET_LIMIT} bytes (2 GiB - 16)'))
        span = 256 // (Ho * Wo) + 2
        if H * W * ldx * 4 * span >= CONV_OFFSET_LIMIT:
            out.append(('input', H * W * ldx * 4 * span, f'the {span} input images one 256-row tile can touch must stay below {CONV_OFFSET_LIMIT} bytes'))
    else:
        tiles, t = (64, 2) if family == 'wino' else (32, 4)
        span = tiles // (-(-H // t) * -(-W // t)) + 2
        for name, ld in (('input', ldx), ('output', ldy), ('residual', ldr)):
            if H * W * ld * 4 * span >= CONV_OFFSET_LIMIT:
                out.append((name, H * W * ld * 4 * span, f'the {span} {name} images one workgroup of {tiles} tiles can touch must stay below {CONV_OFFSET_LIMIT} bytes'))
    return out


def _check_conv(code, entry, family, *shape):
    """_lib.check for a conv entry; a refusal (MYDET_E_UNSUPP) that the tensors' sizes explain names the limit and the byte size."""
    if code == -2:
        broken = conv_size_refusals(family, *shape)
        if broken:
            raise _lib.MydetError(f'{entry} failed: unsupported configuration: ' +
                                  '; '.join(f'{name}: {nbytes} bytes, {rule}' for name, nbytes, rule in broken))
    _lib.check(code, entry)


CONV_FORM_WEIGHTS = {'wino': wino_weights, 'wino4': wino4_weights, 'b3': split_bf16}      # the weight operands derived from the OHWI weight
CONV_FORMS = frozenset(CONV_FORM_WEIGHTS)


def _wino_shape(k, stride, pad, gated):
    return not gated and k == 3 and stride == 1 and tuple(pad) == (1, 1, 1, 1)


def conv_route(B, H, W, Cin, Cout, k, stride, pad, act, *, gated, ldy, ldr, forms, b3_min_rows=None):
    """The launchers `conv2d` tries for a layer, in order, as KernelTimer family names (the keys of CONV_LAUNCHERS): every one but the
    last may answer MYDET_E_UNSUPP.  forms: the weight forms the caller holds (of CONV_FORMS); gated: a squeeze-excite gate multiplies the
    input; ldy / ldr: pixel strides of output and residual (0: none); b3_min_rows: the caller's own row threshold for the split-bf16
    implicit GEMM.  Host code only -- no tensors, no launch -- under the module switches as they are at the call."""
    return _conv_route(_route_switches(), B, H, W, Cin, Cout, k, stride, tuple(pad), act, bool(gated), ldy, ldr,
                       'wino' in forms, 'wino4' in forms, 'b3' in forms, b3_min_rows)


def _route_switches():      # every switch the route reads (p3_takes, b3_takes included): in the memo key, so that a flipped one is obeyed
    return (WINOGRAD, WINOGRAD4, WINO4_MIN_ITEMS, SPLIT_BF16, B3_MIN_ROWS, B3_MIN_FLOP, B3_KPAD, B3_GATED_MIN_COUT, CONV_P3, P3_MIN_WGS,
            P3_S1_MAX_CIN, P3_MIN_FILL)


@functools.lru_cache(maxsize=1 << 14)       # the eager path asks per layer and call
def _conv_route(switches, B, H, W, Cin, Cout, k, stride, pad, act, gated, ldy, ldr, wino, wino4, b3, b3_min_rows):
    Ho, Wo = conv_out_size(H, k, stride, pad[0], pad[2]), conv_out_size(W, k, stride, pad[1], pad[3])
    route = ()
    if b3 and not gated and act in (ACT_NONE, ACT_LEAKY) and p3_takes(B, Ho, Wo, Cin, Cout, k, stride, pad):
        route = ('conv_p3',)
    if WINOGRAD and _wino_shape(k, stride, pad, gated) and ldy % 4 == 0 and ldr % 4 == 0:
        # F(4x4) when the grid fills the chip, or when it is the only Winograd form held
        if wino4 and WINOGRAD4 and (not wino or wino4_items(B, H, W, Cout) >= WINO4_MIN_ITEMS):
            return route + ('conv_wino4',)
        if wino:
            return route + ('conv_wino',)
    if b3 and (not gated or (k == 1 and act == ACT_NONE)) and b3_takes(B * Ho * Wo, Cin, Cout, k, b3_min_rows, B3_GATED_MIN_COUT if gated else 128):
        route += ('conv_igemm_b3',)
    return route + ('conv_igemm',)


def conv_forms(Cout, Cin, k, stride, pad, gated, act, among=CONV_FORMS):
    """The weight forms worth preparing for a layer whose caller may hold the forms `among`: those `conv_route` can name at some batch and
    map size (the row / channel / grid thresholds left open).  The Winograd forms where their weight transforms cover the shape (F(4x4)
    from WINO4_MIN_CIN input channels up); split-bf16 planes under split_bf16's Cin rule -- where a Winograd form takes the layer at
    every size, only up to the channel limit below which conv_p3 comes first."""
    forms = set()
    if WINOGRAD and _wino_shape(k, stride, pad, gated) and Cout % 4 == 0:
        if 'wino' in among and _lib.lib().mydet_wino_weights_floats(Cout, Cin) > 0:
            forms.add('wino')
        if 'wino4' in among and WINOGRAD4 and Cin >= WINO4_MIN_CIN and _lib.lib().mydet_wino4_weights_floats(Cout, Cin) > 0:
            forms.add('wino4')
    if ('b3' in among and SPLIT_BF16 and (Cin % 16 == 0 or (k == 1 and Cin % 4 == 0)) and (not gated or (k == 1 and act == ACT_NONE))
            and (not forms or (k == 3 and Cin <= P3_S1_MAX_CIN and act in (ACT_NONE, ACT_LEAKY)))):
        forms.add('b3')
    return forms


def conv_price(family, B, H, W, Ho, Wo, Cin, Cout, k, residual, interior):
    """(work, nbytes, fused) of one conv launch for KernelTimer.stop: the direct form's FLOPs -- the algorithmic work of the layer, whatever
    the kernel -- and input + output + weights (+ residual) read or written once."""
    b_in, b_out = 4.0 * B * H * W * Cin, 4.0 * B * Ho * Wo * Cout
    b_rest = 4.0 * (k * k * Cin * Cout) + (b_out if residual else 0.0)
    # only conv_igemm discounts a block-interior tensor (fused = None: nbytes); the other families never have: a reported metric, kept
    fused = (0.0 if interior == 'in' else b_in) + (0.0 if interior == 'out' else b_out) + b_rest if family == 'conv_igemm' else None
    return 2.0 * B * Ho * Wo * Cout * k * k * Cin, b_in + b_out + b_rest, fused


# One row per conv kernel family -- a new form is a row here, its predicate in conv_route and its weight rule in conv_forms:
# family (the KernelTimer name): (C entry point, its argument layout, weight form it reads (None: the OHWI weight),
#                                 conv_size_refusals family whose limits explain a refusal)
CONV_LAUNCHERS = {
    'conv_p3': ('mydet_conv3x3_p3_f32', 'p3', 'b3', None),
    'conv_wino4': ('mydet_conv2d_wino4_f32', 'wino', 'wino4', 'wino4'),
    'conv_wino': ('mydet_conv2d_wino_f32', 'wino', 'wino', 'wino'),
    'conv_igemm_b3': ('mydet_conv2d_igemm_b3_f32', 'igemm', 'b3', None),
    'conv_igemm': ('mydet_conv2d_igemm_f32', 'igemm', None, 'igemm'),
}


def _conv_launch(route, c, weights, interior=None, may_refuse=False):
    """Walk `route` through CONV_LAUNCHERS: the first launcher that does not answer MYDET_E_UNSUPP has run the layer (priced for TIMER,
    any other code raised).  The last one's refusal raises too -- unless may_refuse, then None is returned."""
    x, ldx, scale, shift, residual, ldr, gate, out, ldy, B, H, W, Cin, Cout, k, stride, pad, Ho, Wo, act = c
    L = _lib.lib()
    for family in route:
        entry, layout, form, sizes = CONV_LAUNCHERS[family]
        head = (_ptr(x), ldx, _ptr(weights[form]), _ptr(scale), _ptr(shift), _ptr(residual), ldr)
        if layout != 'p3':      # the scratch buffer: F(4x4)'s transform-domain input, or the K-cut tails' partial tiles
            ws = wino4_workspace(x.device, L.mydet_wino4_workspace_bytes(B, H, W, Cin, Cout)) if form == 'wino4' else conv_workspace(x.device)
        t0 = TIMER.start() if TIMER else None
        if layout == 'igemm':
            code = getattr(L, entry)(*head, _ptr(gate), _ptr(ws), ws.numel() * 4, _ptr(out), ldy, B, H, W, Cin, Cout, k, k, stride, pad[0], pad[1],
                                     Ho, Wo, act, _stream())
        elif layout == 'wino':
            code = getattr(L, entry)(*head, _ptr(ws), ws.numel() * 4, _ptr(out), ldy, B, H, W, Cin, Cout, act, _stream())
        else:
            code = getattr(L, entry)(*head, _ptr(out), ldy, B, H, W, Cin, Cout, stride, act, _stream())
        if code == -2 and (may_refuse or family != route[-1]):          # MYDET_E_UNSUPP: the next launcher
            continue
        if t0:
            name = f'{family} {Cin}->{Cout} k{k}s{stride} {H}x{W}' if TIMER_DETAIL else family
            TIMER.stop(name, t0, *conv_price(family, B, H, W, Ho, Wo, Cin, Cout, k, residual is not None, interior))
        if sizes:
            _check_conv(code, entry, sizes, B, H, W, Ho, Wo, ldx, ldy, ldr)
        else:
            _lib.check(code, entry)
        return out
    return None


def _conv_call(x, Cout, scale, shift, k, stride, pad, act, residual, out, out_ld, gate):
    """The tensors of a conv launch in kernel-readable layouts, the output allocated, and its shape: the tuple the launchers unpack."""
    x, ldx = to_nhwc(x)
    B, Cin, H, W = x.shape
    Ho, Wo = conv_out_size(H, k, stride, pad[0], pad[2]), conv_out_size(W, k, stride, pad[1], pad[3])
    if out is None:
        out, ldy = empty_nhwc(B, Cout, Ho, Wo, x.device, out_ld)
    else:
        ldy = nhwc_ld(out)
        assert ldy is not None and out.shape == (B, Cout, Ho, Wo)
    ldr = 0
    if residual is not None:
        residual, ldr = to_nhwc(residual)
        assert residual.shape == out.shape
    return x, ldx, scale, shift, residual, ldr, gate, out, ldy, B, H, W, Cin, Cout, k, stride, pad, Ho, Wo, act


def conv2d(x, w_ohwi, scale, shift, k, stride, pad, act, residual=None, out=None, out_ld=None, gate=None, wino=None,
           wino4=None, interior=None, b3=None, b3_min_rows=None):
    """y = act(conv(x * gate)*scale + shift) + residual.  x logical [B,Cin,H,W]; pad=(top,left,bottom,right);
    gate: optional [B,Cin] per-image channel multipliers (squeeze-excite), 1x1 convs only;
    wino / wino4: optional `wino_weights(w_ohwi)` / `wino4_weights(w_ohwi)`: 3x3 stride-1 pad-1 layers then run a fused
    Winograd kernel -- F(4x4,3x3) when given and the grid fills the chip (or no F(2x2,3x3) weights are given).
    interior: 'in' / 'out' marks the input / output as a tensor that lives only inside a block (bookkeeping of the
    fused-minimum byte count of KernelTimer; no effect on the launch).
    b3: optional `split_bf16(w_ohwi)`: a layer that stays on the direct implicit GEMM then runs it on the bfloat16 matrix
    instructions with float32-exact split operands (include/mydet.h: mydet_conv2d_igemm_b3_f32; Cin % 16 == 0; with a gate: 1x1 layers
    without activation), from B3_MIN_ROWS output pixels up (`b3_min_rows` overrides).  Which launcher runs: `conv_route`."""
    require_gpu(x, 'conv2d')
    if x.shape[1] % 4:
        raise ValueError(f'conv2d: Cin = {x.shape[1]} is not a multiple of 4 (the implicit-GEMM kernel reads channels in '
                         'float4; the 3-channel image layer goes through conv2d_stem)')
    c = _conv_call(x, w_ohwi.shape[0], scale, shift, k, stride, pad, act, residual, out, out_ld, gate)
    weights = {None: w_ohwi, 'wino': wino, 'wino4': wino4, 'b3': b3}
    # conv_route, with the forms held as its memoised core takes them
    ldr, ldy, (B, H, W, Cin, Cout) = c[5], c[8], c[9:14]
    route = _conv_route(_route_switches(), B, H, W, Cin, Cout, k, stride, tuple(pad), act, gate is not None, ldy, ldr,
                        wino is not None, wino4 is not None, b3 is not None, b3_min_rows)
    return _conv_launch(route, c, weights, interior)


def conv3x3_p3(x, b3, scale, shift, stride, act, residual=None, out=None, out_ld=None, cout=None):
    """y = act(conv3x3_pad1(x) * scale + shift) + residual on the patch-resident split-bf16 kernel (csrc/conv_p3.hip,
    include/mydet.h: mydet_conv3x3_p3_f32).  b3 = split_bf16(w_ohwi) of the [Cout, 3, 3, Cin] weight; cout = Cout (default: len(shift)).
    Returns None when the kernel does not cover the shape (Cin % 16, activation): the caller then uses conv2d."""
    require_gpu(x, 'conv3x3_p3')
    if x.shape[1] % 16 or stride not in (1, 2) or act not in (ACT_NONE, ACT_LEAKY) or b3 is None:
        return None
    Cout = int(cout if cout is not None else (shift if shift is not None else scale).shape[0])
    c = _conv_call(x, Cout, scale, shift, 3, stride, (1, 1, 1, 1), act, residual, out, out_ld, None)
    return _conv_launch(('conv_p3',), c, {'b3': b3}, may_refuse=True)


def conv2d_stem(x, w_ohwi, scale, shift, stride, pad, act):
    """3->32 3x3 first layer; reads x with its own strides (NCHW or channels-last)."""
    require_gpu(x, 'conv2d_stem')
    assert x.dtype == torch.float32 and x.shape[1] == 3
    B, _, H, W = x.shape
    Cout = w_ohwi.shape[0]
    Ho = conv_out_size(H, 3, stride, pad[0], pad[2])
    Wo = conv_out_size(W, 3, stride, pad[1], pad[3])
    out, ldy = empty_nhwc(B, Cout, Ho, Wo, x.device)
    sb, sc, sh, sw = x.stride()
    t0 = TIMER.start() if TIMER else None
    code = _lib.lib().mydet_conv2d_stem_f32(_ptr(x), sb, sc, sh, sw, _ptr(w_ohwi), _ptr(scale), _ptr(shift),
                                            _ptr(out), ldy, B, H, W, Cout, stride, pad[0], pad[1], Ho, Wo, act,
                                            _stream())
    if t0:
        TIMER.stop('conv_stem', t0, *[4.0 * B * (3 * H * W + Cout * Ho * Wo)] * 2)        # bytes moved
    _lib.check(code, 'mydet_conv2d_stem_f32')
    return out


# MYDET_STEM_P3=0 keeps Darknet-53's stem and its first stride-2 conv as two launches (A/B measurements).  The fused launch measured
# faster at every size tried (profiles/stem_p3_fused.md: batch 32 at 640^2 1 242 -> 1 044 us, at 512^2 813 -> 685 us; batch 1 at
# 512^2, 512 workgroups, 47 -> 29 us), so there is no size bound beyond conv_p3's own
STEM_P3 = os.environ.get('MYDET_STEM_P3', '1') != '0'


def stem_p3_plan(B, Hs, Ws, Cout):
    """(workgroups, dynamic LDS bytes per workgroup) of mydet_conv_stem_p3_f32 (csrc/conv_stem_p3.hip) for a stem map of Hs x Ws: 8 x 16
    output tiles x 64 channels; one 16-channel slab of the 17 x 36-position stride-2 patch in three bf16 planes + the 19 x 36 x 3
    float32 image patch."""
    Ho, Wo = (Hs - 1) // 2 + 1, (Ws - 1) // 2 + 1
    return B * -(-Ho // 8) * -(-Wo // 16) * (Cout // 64), 3 * 17 * 36 * 32 + 3 * 19 * 36 * 4


def stem_p3_takes(B, H, W, Cout, pad0):
    """True when Darknet-53's first two layers take the fused launch: the second layer would run conv_p3's 8 x 16 tiles anyway (no strip
    tiles); measured faster than the two launches at every such size tried (profiles/stem_p3_fused.md)."""
    Hs, Ws = conv_out_size(H, 3, 1, pad0[0], pad0[2]), conv_out_size(W, 3, 1, pad0[1], pad0[3])
    Ho, Wo = (Hs - 1) // 2 + 1, (Ws - 1) // 2 + 1
    if not STEM_P3 or Cout % 64 or not p3_takes(B, Ho, Wo, 32, Cout, 3, 2, (1, 1, 1, 1)):
        return False
    return p3_plan(Ho, Wo, Cout, 2).strip == 0


def stem_p3_weights(w_ohwi):
    """The stem operand of `conv_stem_p3`: the OHWI stem weight [32, 3, 3, 3] with every row's K = 27 zero-padded to 32, as
    `split_bf16` planes."""
    w = torch.zeros((w_ohwi.shape[0], 1, 1, 32), dtype=torch.float32, device=w_ohwi.device)
    w[:, 0, 0, :27] = w_ohwi.reshape(w_ohwi.shape[0], 27).float()
    return split_bf16(w)


def conv_stem_p3(x, w0_planes, scale0, shift0, pad0, w1_planes, scale1, shift1, act0=ACT_LEAKY, act1=ACT_LEAKY, out=None, out_ld=None):
    """y = act1(BN1(conv3x3_s2_pad1(act0(BN0(conv3x3_s1(image)))))) in one launch (csrc/conv_stem_p3.hip, include/mydet.h:
    mydet_conv_stem_p3_f32): the 32-channel stem map is never written.  x [B,3,H,W] in any strides; w0_planes =
    stem_p3_weights(stem OHWI weight), w1_planes = split_bf16 of the second layer's [Cout,3,3,32] weight; pad0 = the stem's (top,
    left, bottom, right).  Returns None when the kernel does not cover the arguments: the caller then uses conv2d_stem + conv2d."""
    require_gpu(x, 'conv_stem_p3')
    assert x.dtype == torch.float32 and x.shape[1] == 3
    B, _, H, W = x.shape
    Cout = int(shift1.shape[0])
    Hs, Ws = conv_out_size(H, 3, 1, pad0[0], pad0[2]), conv_out_size(W, 3, 1, pad0[1], pad0[3])
    Ho, Wo = (Hs - 1) // 2 + 1, (Ws - 1) // 2 + 1
    if out is None:
        out, ldy = empty_nhwc(B, Cout, Ho, Wo, x.device, out_ld)
    else:
        ldy = nhwc_ld(out)
        assert ldy is not None and out.shape == (B, Cout, Ho, Wo)
    sb, sc, sh, sw = x.stride()
    t0 = TIMER.start() if TIMER else None
    code = _lib.lib().mydet_conv_stem_p3_f32(_ptr(x), sb, sc, sh, sw, _ptr(w0_planes), _ptr(scale0), _ptr(shift0), act0, _ptr(w1_planes),
                                             _ptr(scale1), _ptr(shift1), act1, _ptr(out), ldy, B, H, W, 32, Cout, 1, pad0[0], pad0[1],
                                             Hs, Ws, 2, _stream())
    if code == -2:
        return None
    if t0:      # algorithmic FLOPs and bytes of the two reference layers: stem (image in, map out) + stride-2 conv (map in, out, weights)
        b_img, b_map, b_out = 4.0 * B * 3 * H * W, 4.0 * B * 32 * Hs * Ws, 4.0 * B * Cout * Ho * Wo
        TIMER.stop('conv_stem_p3', t0, 2.0 * B * (Hs * Ws * 32 * 27 + Ho * Wo * Cout * 9 * 32), b_img + 2 * b_map + b_out + 4.0 * 9 * 32 * Cout,
                   fused=b_img + b_out + 4.0 * 9 * 32 * Cout)
    _lib.check(code, 'mydet_conv_stem_p3_f32')
    return out


def se_slices(n_pixels):
    """Number of pixel slices the SE average is split over (deterministic two-stage sum)."""
    return max(1, min(128, n_pixels // 16))


def dwconv(x, w_kkc, scale, shift, k, stride, pad, act, squeeze=False, interior=False, se=None):
    """Depthwise k x k conv, y = act(conv*scale + shift); w_kkc [k,k,C]; pad=(top,left,bottom,right).
    squeeze=True also returns the per-slice channel sums [B,S,C] of y (input of `se_gate`).
    se=(w1 [Cse,C], b1 [Cse], w2t [Cse,C], b2 [C]): the launch also finishes the squeeze-excite gate of y
    (include/mydet.h: mydet_se_tail) and (y, gate [B,C]) is returned -- no squeeze sums, no gate launch."""
    require_gpu(x, 'dwconv')
    x, ldx = to_nhwc(x)
    B, C, H, W = x.shape
    Ho = conv_out_size(H, k, stride, pad[0], pad[2])
    Wo = conv_out_size(W, k, stride, pad[1], pad[3])
    out, ldy = empty_nhwc(B, C, Ho, Wo, x.device)
    partial, S = None, 0
    if squeeze or se is not None:
        S = _lib.lib().mydet_dwconv_slices(Ho, Wo, C, k, stride)      # what the kernel chosen for this layer writes
    if squeeze:
        partial = torch.empty((B, S + 1, C), dtype=torch.float32, device=x.device)    # slice S: scratch for the mean
    tail, gate, keep = _se_tail(se, B, C, _lib.lib().mydet_dwconv_se_groups(Ho, Wo, C, k, stride) if se is not None else 0, x.device)
    t0 = TIMER.start() if TIMER else None
    code = _lib.lib().mydet_dwconv_f32(_ptr(x), ldx, _ptr(w_kkc), _ptr(scale), _ptr(shift), _ptr(out), ldy, B, H, W, C,
                                       k, stride, pad[0], pad[1], Ho, Wo, act, _ptr(partial), S,
                                       ctypes.byref(tail) if tail is not None else None, _stream())
    if t0:
        TIMER.stop(f'dwconv {C} k{k}s{stride} {H}x{W}' if TIMER_DETAIL else 'dwconv', t0, *[4.0 * B * C * (H * W + Ho * Wo)] * 2,
                   fused=0.0 if interior is True else (4.0 * B * C * H * W if interior == 'out' else None))
    _lib.check(code, 'mydet_dwconv_f32')
    if se is not None:
        return out, gate
    return (out, partial) if squeeze else out


# (k, stride, Cin) the blocks use the fused launch for: the instantiated shapes where it beats expand + depthwise
# (tools/bench_mbconv.py, batch 16: 235 vs 386, 168 vs 243, 177 vs 192 us; (5,1,40) and (3,2,40) exist but lose: 145 vs 127, 95 vs 73)
MBCONV_FUSED_SHAPES = {(3, 2, 16), (3, 1, 24), (5, 2, 24)}
# MYDET_FUSED_MBCONV=0 keeps expand conv and depthwise conv as two launches (A/B measurements)
FUSED_MBCONV = os.environ.get('MYDET_FUSED_MBCONV', '1') != '0'


def fold_scale(w, scale):
    """Conv weight with the per-output-channel BatchNorm scale multiplied in (w OHWI [Cout,...] or depthwise [k,k,C])."""
    if w.dim() == 3:
        return (w * scale.view(1, 1, -1)).contiguous()
    return (w * scale.view(-1, *([1] * (w.dim() - 1)))).contiguous()


def mbconv_expand_dw(x, w_expand, shift0, w_dw, shift1, k, stride, pad, se=None):
    """swish(BN1(depthwise_k(swish(BN0(expand1x1(x)))))) and the per-tile channel sums of the result (SE squeeze) in
    one launch; w_expand OHWI [Cexp,1,1,Cin] and w_dw [k,k,Cexp] carry the BatchNorm scales (`fold_scale`), shift0 /
    shift1 are the folded shifts; pad=(top,left,bottom,right) of the expanded map.
    Returns (y [B,Cexp,Ho,Wo], partial [B,S+1,Cexp]) -- or, with se=(w1, b1, w2t, b2) as in `dwconv`, (y, gate [B,Cexp]):
    the launch finishes the squeeze-excite gate itself."""
    require_gpu(x, 'mbconv_expand_dw')
    x, ldx = to_nhwc(x)
    B, Cin, H, W = x.shape
    Cexp = w_expand.shape[0]
    Ho = conv_out_size(H, k, stride, pad[0], pad[2])
    Wo = conv_out_size(W, k, stride, pad[1], pad[3])
    out, ldy = empty_nhwc(B, Cexp, Ho, Wo, x.device)
    S = _lib.lib().mydet_mbconv_tiles(Ho, Wo, stride)
    partial = torch.empty((B, S + 1, Cexp), dtype=torch.float32, device=x.device) if se is None else None
    tail, gate, keep = _se_tail(se, B, Cexp, S, x.device)
    t0 = TIMER.start() if TIMER else None
    code = _lib.lib().mydet_mbconv_expand_dw_f32(_ptr(x), ldx, _ptr(w_expand), _ptr(shift0), _ptr(w_dw),
                                                 _ptr(shift1), _ptr(out), ldy, B, H, W, Cin, Cexp, k, stride,
                                                 pad[0], pad[1], Ho, Wo, _ptr(partial), S,
                                                 ctypes.byref(tail) if tail is not None else None, _stream())
    if t0:      # algorithmic bytes of the two reference layers it replaces: expand (in + out) and depthwise (in + out)
        nb = 4.0 * B * (H * W * (Cin + Cexp) + Cexp * (H * W + Ho * Wo))
        TIMER.stop(f'mbconv_expand_dw {Cin}->{Cexp} k{k}s{stride} {H}x{W}' if TIMER_DETAIL else 'mbconv_expand_dw', t0,
                   2.0 * B * H * W * Cin * Cexp, nb, fused=4.0 * B * H * W * Cin)
    _lib.check(code, 'mydet_mbconv_expand_dw_f32')
    return (out, gate) if se is not None else (out, partial)


# MYDET_FUSED_STEM=0 keeps the EfficientNet stem and block 0's depthwise conv as two launches
FUSED_STEM_DW = os.environ.get('MYDET_FUSED_STEM', '1') != '0'


def stem_dw(x, w_stem, shift0, w_dw, shift1, pad, se=None):
    """swish(BN1(depthwise3x3(swish(BN0(conv3x3_s2(image)))))) and the per-tile channel sums of the result in one launch
    (EfficientNet stem + block 0's depthwise conv).  x [B,3,H,W] in any strides; w_stem OHWI [32,3,3,3] and w_dw
    [3,3,32] carry the BatchNorm scales (`fold_scale`); pad = the stem's (top, left, bottom, right).
    Returns (y [B,32,Hs,Ws], partial [B,S+1,32]) -- or, with se=(w1, b1, w2t, b2) as in `dwconv`, (y, gate [B,32])."""
    require_gpu(x, 'stem_dw')
    assert x.dtype == torch.float32 and x.shape[1] == 3
    B, _, H, W = x.shape
    C = w_stem.shape[0]
    Hs = conv_out_size(H, 3, 2, pad[0], pad[2])
    Ws = conv_out_size(W, 3, 2, pad[1], pad[3])
    out, ldy = empty_nhwc(B, C, Hs, Ws, x.device)
    S = _lib.lib().mydet_mbconv_tiles(Hs, Ws, 1)
    partial = torch.empty((B, S + 1, C), dtype=torch.float32, device=x.device) if se is None else None
    tail, gate, keep = _se_tail(se, B, C, S, x.device)
    sb, sc, sh, sw = x.stride()
    t0 = TIMER.start() if TIMER else None
    code = _lib.lib().mydet_stem_dw_f32(_ptr(x), sb, sc, sh, sw, _ptr(w_stem), _ptr(shift0), _ptr(w_dw), _ptr(shift1), _ptr(out),
                                        ldy, B, H, W, C, pad[0], pad[1], Hs, Ws, _ptr(partial), S,
                                        ctypes.byref(tail) if tail is not None else None, _stream())
    if t0:      # reference-layer bytes: stem (image in, map out) + depthwise (map in, map out)
        TIMER.stop('stem_dw', t0, 0.0, 4.0 * B * (3 * H * W + 3 * C * Hs * Ws), fused=4.0 * B * (3 * H * W + C * Hs * Ws))
    _lib.check(code, 'mydet_stem_dw_f32')
    return (out, gate) if se is not None else (out, partial)


def channel_sums(x):
    """Per-slice channel sums [B,S,C] of x [B,C,H,W] (standalone squeeze)."""
    require_gpu(x, 'channel_sums')
    x, ldx = to_nhwc(x)
    B, C, H, W = x.shape
    S = se_slices(H * W)
    partial = torch.empty((B, S + 1, C), dtype=torch.float32, device=x.device)
    code = _lib.lib().mydet_channel_sums_f32(_ptr(x), ldx, B, H, W, C, _ptr(partial), S, _stream())
    _lib.check(code, 'mydet_channel_sums_f32')
    return partial


def se_gate(partial, n_pixels, w1, b1, w2t, b2):
    """gate [B,C] = sigmoid(W2 . swish(W1 . mean + b1) + b2) from per-slice sums [B,S+1,C]; w2t = W2 transposed [Cse,C]."""
    require_gpu(partial, 'se_gate')
    B, S, C = partial.shape
    S -= 1
    Cse = w1.shape[0]
    gate = torch.empty((B, C), dtype=torch.float32, device=partial.device)
    t0 = TIMER.start() if TIMER else None
    code = _lib.lib().mydet_se_gate_f32(_ptr(partial), S, B, n_pixels, C, _ptr(w1), _ptr(b1), Cse, _ptr(w2t), _ptr(b2),
                                        _ptr(gate), _stream())
    if t0:
        TIMER.stop('se_gate', t0, *[4.0 * B * S * C] * 2, fused=0.0)
    _lib.check(code, 'mydet_se_gate_f32')
    return gate


def maxpool3s2(x):
    """max_pool2d(x, kernel_size=3, stride=2, padding=1)."""
    require_gpu(x, 'maxpool3s2')
    x, ldx = to_nhwc(x)
    B, C, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out, ldy = empty_nhwc(B, C, Ho, Wo, x.device)
    t0 = TIMER.start() if TIMER else None
    code = _lib.lib().mydet_maxpool3s2_f32(_ptr(x), ldx, _ptr(out), ldy, B, H, W, C, Ho, Wo, _stream())
    if t0:
        TIMER.stop('maxpool', t0, *[4.0 * B * C * (H * W + Ho * Wo)] * 2)
    _lib.check(code, 'mydet_maxpool3s2_f32')
    return out


FUSE_SAME, FUSE_UP2X, FUSE_POOL = 0, 1, 2


def bifpn_fuse(inputs, modes, weights):
    """swish(sum_i w_i * in_i) with w = relu(weights)/(sum+1e-4).  inputs: 2-3 tensors; modes[i] in
    FUSE_SAME / FUSE_UP2X (half-size map, nearest 2x) / FUSE_POOL (double-size map, max-pool 3/2/1).
    The output has the size of the FUSE_SAME input(s)."""
    n = len(inputs)
    require_gpu(inputs[0], 'bifpn_fuse')
    prepared = [to_nhwc(t) for t in inputs]
    ref = next(t for (t, _), m in zip(prepared, modes) if m == FUSE_SAME)
    B, C, H, W = ref.shape
    for (t, _), m in zip(prepared, modes):
        exp = {FUSE_SAME: (H, W), FUSE_UP2X: (H // 2, W // 2), FUSE_POOL: (H * 2, W * 2)}[m]
        assert tuple(t.shape) == (B, C) + exp, (tuple(t.shape), m, (B, C, H, W))
    out, ldy = empty_nhwc(B, C, H, W, ref.device)
    args = []
    for i in range(3):
        if i < n:
            args += [_ptr(prepared[i][0]), prepared[i][1], int(modes[i])]
        else:
            args += [ctypes.c_void_p(0), 0, 0]
    t0 = TIMER.start() if TIMER else None
    code = _lib.lib().mydet_bifpn_fuse_f32(n, *args, _ptr(weights), _ptr(out), ldy, B, H, W, C, _stream())
    if t0:
        TIMER.stop('bifpn_fuse', t0, *[4.0 * B * C * H * W * (n + 1)] * 2)
    _lib.check(code, 'mydet_bifpn_fuse_f32')
    return out


def pack_pointwise(w):
    """Pointwise weight [Cout, C] (or OHWI [Cout,1,1,C]) in the MFMA operand order `sepconv_nodes` reads, four k-steps of
    a lane side by side (one 16-byte load / LDS read per four MFMAs; include/mydet.h):
        packed[nb][kq][lane][e] = W[16*nb + (lane & 15)][4*(4*kq + e) + (lane >> 4)],   kq < ceil(C/16),
    zero for rows >= Cout and k >= C."""
    w = w.reshape(w.shape[0], -1).float()
    Cout, C = w.shape
    assert C % 4 == 0
    nb, ks = (Cout + 15) // 16, C // 4
    kq = (ks + 3) // 4
    wp = w.new_zeros((nb * 16, kq * 4, 4))                 # [row][k-step][k within the step]
    wp[:Cout, :ks] = w.view(Cout, ks, 4)
    # [nb][16 rows][kq][e][4 kk] -> [nb][kq][kk][16 rows][e]: lane = kk * 16 + row
    return wp.view(nb, 16, kq, 4, 4).permute(0, 2, 4, 1, 3).contiguous().view(nb, kq, 64, 4)


SEPCONV_CHANNELS = (88,)        # instantiated channel counts of the fused node kernel
# MYDET_FUSED_NODES=0 keeps the pyramid on the three-launch path (fusion, depthwise, pointwise GEMM): A/B measurements
FUSED_NODES = os.environ.get('MYDET_FUSED_NODES', '1') != '0'


def sepconv_nodes(nodes):
    """Fused [fusion + swish ->] depthwise 3x3 -> pointwise 1x1 (+ folded BN, act) nodes, up to 10 per launch.
    nodes: list of dicts with keys inputs (1-3 tensors [B,C,h,w]), modes (FUSE_*), fuse_weights (raw, for >= 2 inputs),
    w_dw [3,3,C], w_pw (pack_pointwise), scale (or None), shift, cout, act, and optionally out (a tensor to write).
    Returns the output tensors."""
    assert 1 <= len(nodes) <= _lib.SEPCONV_MAX_NODES
    arr = (_lib.SepconvNode * len(nodes))()
    outs, keep = [], []
    B = C = None
    work = fused = 0.0
    for i, nd in enumerate(nodes):
        prepared = [to_nhwc(t) for t in nd['inputs']]
        require_gpu(prepared[0][0], 'sepconv_nodes')
        modes = list(nd.get('modes') or [FUSE_SAME] * len(prepared))
        ref = next(t for (t, _), m in zip(prepared, modes) if m == FUSE_SAME)
        b, c, H, W = ref.shape
        B, C = (b, c) if B is None else (B, C)
        assert (b, c) == (B, C), 'all nodes of a launch share batch and channels'
        for (t, _), m in zip(prepared, modes):
            exp = {FUSE_SAME: (H, W), FUSE_UP2X: (H // 2, W // 2), FUSE_POOL: (H * 2, W * 2)}[m]
            assert tuple(t.shape) == (B, C) + exp, (tuple(t.shape), m, (B, C, H, W))
        cout = nd['cout']
        out = nd.get('out')
        if out is None:
            out, ldy = empty_nhwc(B, cout, H, W, ref.device)
        else:
            ldy = nhwc_ld(out)
            assert ldy is not None and tuple(out.shape) == (B, cout, H, W)
        n_in = len(prepared)
        node = arr[i]
        for k in range(3):
            node.inp[k] = prepared[k][0].data_ptr() if k < n_in else None
            node.ld[k] = prepared[k][1] if k < n_in else 0
            node.mode[k] = int(modes[k]) if k < n_in else 0
        node.n_in = n_in
        fw = nd.get('fuse_weights')
        node.fuse_weights = fw.data_ptr() if n_in > 1 else None
        node.w_dw, node.w_pw_packed = nd['w_dw'].data_ptr(), nd['w_pw'].data_ptr()
        node.scale = nd['scale'].data_ptr() if nd.get('scale') is not None else None
        node.shift = nd['shift'].data_ptr()
        node.y, node.ldy, node.H, node.W, node.Cout, node.act = out.data_ptr(), ldy, H, W, cout, int(nd.get('act', ACT_NONE))
        keep.append((prepared, fw, out))
        outs.append(out)
        # algorithmic bytes of the reference layers this node replaces: fusion (n+1 maps), depthwise (2), pointwise (C + Cout)
        px = 4.0 * B * H * W
        work += px * ((C * (n_in + 1) if n_in > 1 else 0) + 2 * C + C + cout)
        fused += sum(4.0 * t.numel() for t, _ in prepared) + px * cout
    t0 = TIMER.start() if TIMER else None
    code = _lib.lib().mydet_sepconv_nodes_f32(len(nodes), ctypes.cast(arr, ctypes.c_void_p), B, C, _stream())
    if t0:
        TIMER.stop('sepconv_nodes', t0, work, work, fused=fused)
    _lib.check(code, 'mydet_sepconv_nodes_f32')
    return outs


def pack_lr_tb(w_lr0, w_tb0, w_lr1, b_lr1, w_tb1, b_tb1):
    """Kernel-ready weights of one _LR_TB_last layer (mydet_lr_tb_levels_f32): (30 C + 4) floats, the two depthwise convs
    [C,1,3,3] as [kh][kw][C], the (1,3) / (3,1) convs [2,C,1,3] / [2,C,3,1] as [o][k][C], then the biases in ltrb order."""
    C = w_lr0.shape[0]
    with torch.no_grad():
        parts = [w_lr0.reshape(C, 9).t(), w_tb0.reshape(C, 9).t(), w_lr1[:, :, 0, :].permute(0, 2, 1),
                 w_tb1[:, :, :, 0].permute(0, 2, 1), torch.stack([b_lr1[0], b_tb1[0], b_lr1[1], b_tb1[1]])]
        return torch.cat([p.detach().float().reshape(-1) for p in parts]).contiguous()


def lr_tb_levels(levels):
    """The lr_tb box layer (models/rpns.py _LR_TB_last) of up to 8 pyramid levels in ONE launch.  levels: list of
    (x [B,C,H,W], packed weights from pack_lr_tb); all share B and C.  Returns per level the box logits [B,4,H,W]
    (l, t, r, b), stored pixel-major [B,H,W,4]."""
    assert 1 <= len(levels) <= _lib.LR_TB_MAX_LEVELS
    arr = (_lib.LrTbLevel * len(levels))()
    outs, keep = [], []
    B = C = None
    nbytes = flops = 0.0
    for i, (x, w) in enumerate(levels):
        require_gpu(x, 'lr_tb_levels')
        xt, ldx = to_nhwc(x)
        b, c, H, W = xt.shape
        B, C = (b, c) if B is None else (B, C)
        assert (b, c) == (B, C), 'all levels of a launch share batch and channels'
        assert w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and w.numel() == 30 * C + 4
        out, ldy = empty_nhwc(B, 4, H, W, xt.device)
        lv = arr[i]
        lv.x, lv.ldx, lv.w, lv.y, lv.ldy, lv.H, lv.W = xt.data_ptr(), ldx, w.data_ptr(), out.data_ptr(), ldy, H, W
        keep.append((xt, w, out))
        outs.append(out)
        nbytes += 4.0 * B * H * W * (C + 4)                       # the map read once, ltrb written once
        flops += 2.0 * B * H * W * C * 30                             # 2 x depthwise 3x3, 2 x (2 outputs x 3 taps)
    t0 = TIMER.start() if TIMER else None
    code = _lib.lib().mydet_lr_tb_levels_f32(len(levels), ctypes.cast(arr, ctypes.c_void_p), B, C, _stream())
    if t0:
        TIMER.stop('lr_tb', t0, flops, nbytes)
    _lib.check(code, 'mydet_lr_tb_levels_f32')
    return outs


# MYDET_FUSED_DECODE=0: the EfDetHead + RetinaLayer path writes its class logits and decodes them in a second launch
FUSED_DECODE = os.environ.get('MYDET_FUSED_DECODE', '1') != '0'


def pack_pointwise_per_anchor(w, shift, A, n_cls):
    """Class-tower weights [A * n_cls, C] / shifts [A * n_cls] with every anchor's rows padded to whole 16-channel blocks
    (zero rows / zero shifts), in `pack_pointwise` order: what `sepconv_decode_retina` reads (include/mydet.h)."""
    w = w.reshape(w.shape[0], -1).float()
    C = w.shape[1]
    cpad = (n_cls + 15) // 16 * 16
    wp = w.new_zeros((A, cpad, C))
    wp[:, :n_cls] = w.view(A, n_cls, C)
    sp = shift.new_zeros((A, cpad))
    sp[:, :n_cls] = shift.float().view(A, n_cls)
    return pack_pointwise(wp.view(A * cpad, C)), sp.view(-1).contiguous()


def sepconv_decode_retina(nodes, A, n_cls, img_hw, bbox, class_idx, score):
    """The last sepconv of every EfDetHead tower with RetinaLayer's decode in its epilogue, one launch.
    nodes: dicts with keys inputs ([tensor [B,C,h,w]]), w_dw, w_pw, shift, scale (or None), kind (0 class tower: w_pw /
    shift from `pack_pointwise_per_anchor`; 1 box tower: plain `pack_pointwise`), stride, anchors_wh ([A,2], box
    towers), n_off.  Writes bbox [B,N,4], class_idx [B,N] i64, score [B,N] at the nodes' candidate ranges."""
    assert 1 <= len(nodes) <= _lib.SEPCONV_MAX_NODES
    require_gpu(bbox, 'sepconv_decode_retina')
    arr = (_lib.SepconvDecodeNode * len(nodes))()
    keep = []
    B = C = None
    work = fused = 0.0
    cpad = (n_cls + 15) // 16 * 16
    for i, nd in enumerate(nodes):
        x, ld = to_nhwc(nd['inputs'][0])
        b, c, H, W = x.shape
        B, C = (b, c) if B is None else (B, C)
        assert (b, c) == (B, C), 'all nodes of a launch share batch and channels'
        node = arr[i].node
        for k in range(3):
            node.inp[k] = x.data_ptr() if k == 0 else None
            node.ld[k] = ld if k == 0 else 0
            node.mode[k] = 0
        node.n_in = 1
        node.fuse_weights = None
        node.w_dw, node.w_pw_packed = nd['w_dw'].data_ptr(), nd['w_pw'].data_ptr()
        node.scale = nd['scale'].data_ptr() if nd.get('scale') is not None else None
        node.shift = nd['shift'].data_ptr()
        node.y, node.ldy, node.H, node.W, node.act = None, 0, H, W, ACT_NONE
        node.Cout = A * cpad if nd['kind'] == 0 else A * 4
        arr[i].kind, arr[i].stride, arr[i].n_off = int(nd['kind']), float(nd['stride']), int(nd['n_off'])
        anch = None
        if nd['kind'] == 1:
            anch = np.ascontiguousarray(np.asarray(nd['anchors_wh'], dtype=np.float32).reshape(-1))
            assert anch.size == 2 * A
        arr[i].anchors_wh = anch.ctypes.data if anch is not None else None
        keep.append((x, anch))
        # reference-layer bytes: depthwise (2 maps), pointwise (C in, Cout out), decode (Cout in, 28 B per candidate out)
        px = 4.0 * B * H * W
        cout = A * n_cls if nd['kind'] == 0 else A * 4
        work += px * (2 * C + C + cout + cout) + (12.0 if nd['kind'] == 0 else 16.0) * B * A * H * W
        fused += px * C + (12.0 if nd['kind'] == 0 else 16.0) * B * A * H * W
    t0 = TIMER.start() if TIMER else None
    code = _lib.lib().mydet_sepconv_decode_retina_f32(len(nodes), ctypes.cast(arr, ctypes.c_void_p), B, C, A, n_cls,
                                                      int(img_hw[0]), int(img_hw[1]), _ptr(bbox), _ptr(class_idx),
                                                      _ptr(score), bbox.shape[1], _stream())
    if t0:
        TIMER.stop('sepconv_decode', t0, work, work, fused=fused)
    _lib.check(code, 'mydet_sepconv_decode_retina_f32')


def upsample_concat(a, size, b=None):
    """cat((nearest_resize(a, size), b), dim=1) in one pass."""
    require_gpu(a, 'upsample_concat')
    a, lda = to_nhwc(a)
    B, C1, Ha, Wa = a.shape
    Ho, Wo = size
    C2, ldb = 0, 0
    if b is not None:
        b, ldb = to_nhwc(b)
        C2 = b.shape[1]
        assert b.shape[0] == B and tuple(b.shape[2:]) == (Ho, Wo)
    out, ldy = empty_nhwc(B, C1 + C2, Ho, Wo, a.device)
    t0 = TIMER.start() if TIMER else None
    code = _lib.lib().mydet_upsample_concat_f32(_ptr(a), lda, Ha, Wa, C1, _ptr(b), ldb, C2, _ptr(out), ldy, B, Ho,
                                                Wo, _stream())
    if t0:
        TIMER.stop('upsample_concat', t0, *[4.0 * B * (C1 * Ha * Wa + C2 * Ho * Wo + (C1 + C2) * Ho * Wo)] * 2)
    _lib.check(code, 'mydet_upsample_concat_f32')
    return out


# MYDET_FUSED_UPCAT=0 keeps nearest-upsample + concat and the 1x1 conv behind them as two launches (A/B measurements)
FUSED_UPCAT = os.environ.get('MYDET_FUSED_UPCAT', '1') != '0'


def conv1x1_upcat(a, b, w_ohwi, scale, shift, act):
    """act(conv1x1(cat((nearest_2x(a), b), dim=1)) * scale + shift) in ONE launch -- the concatenated tensor is read on the
    fly, never written; bit-identical to `upsample_concat` + `conv2d` for every shape it accepts.  a [B,C1,H/2,W/2],
    b [B,C2,H,W].  Returns None when the shape is not covered -- channel counts not multiples of 32, or a shape `conv2d` would
    not run on the 64 x 64 x 32 tile the fused launch is instantiated for (include/mydet.h) -- and the caller then runs the two
    launches."""
    require_gpu(a, 'conv1x1_upcat')
    B, C1, Ha, Wa = a.shape
    _, C2, H, W = b.shape
    Cout = w_ohwi.shape[0]
    if not FUSED_UPCAT or (H, W) != (2 * Ha, 2 * Wa) or C1 % 32 or C2 % 32 or act != ACT_LEAKY or w_ohwi.shape[1:3] != (1, 1):
        return None
    a, lda = to_nhwc(a)
    b, ldb = to_nhwc(b)
    out, ldy = empty_nhwc(B, Cout, H, W, a.device)
    ws = conv_workspace(a.device)
    t0 = TIMER.start() if TIMER else None
    code = _lib.lib().mydet_conv1x1_upcat_f32(_ptr(a), lda, C1, _ptr(b), ldb, C2, _ptr(w_ohwi), _ptr(scale), _ptr(shift), _ptr(ws),
                                              ws.numel() * 4, _ptr(out), ldy, B, H, W, Cout, act, _stream())
    if code == -2:                                  # MYDET_E_UNSUPP: the caller runs the two launches
        return None
    if t0:
        name = f'conv_igemm {C1}^+{C2}->{Cout} k1s1 {H}x{W}' if TIMER_DETAIL else 'conv_igemm'
        work, nbytes, _ = conv_price('conv_igemm', B, H, W, H, W, C1 + C2, Cout, 1, False, None)
        TIMER.stop(name, t0, work, nbytes - 4.0 * B * 3 * Ha * Wa * C1)      # `a` is read once at half resolution, not as its 2x copy
    _lib.check(code, 'mydet_conv1x1_upcat_f32')
    return out


def space_to_depth(x):
    """Focus' 2x2 space-to-depth (external/ultralytics/common.py:84-86): [B,C,H,W] (any strides) -> [B,4C,H/2,W/2]
    channels-last, channel g*C + c with g = 0:(dy 0,dx 0) 1:(1,0) 2:(0,1) 3:(1,1)."""
    require_gpu(x, 'space_to_depth')
    assert x.dtype == torch.float32 and x.dim() == 4
    B, C, H, W = x.shape
    assert H % 2 == 0 and W % 2 == 0
    out, ldy = empty_nhwc(B, 4 * C, H // 2, W // 2, x.device)
    sb, sc, sh, sw = x.stride()
    t0 = TIMER.start() if TIMER else None
    code = _lib.lib().mydet_space_to_depth_f32(_ptr(x), sb, sc, sh, sw, _ptr(out), ldy, B, C, H, W, _stream())
    if t0:
        TIMER.stop('space_to_depth', t0, *[8.0 * B * C * H * W] * 2)
    _lib.check(code, 'mydet_space_to_depth_f32')
    return out


def spp_concat(x, ks=(5, 9, 13)):
    """cat([x] + [max_pool2d(x, k, 1, k // 2) for k in ks], 1) in one pass (external/ultralytics/common.py:68-70)."""
    require_gpu(x, 'spp_concat')
    assert len(ks) == 3
    x, ldx = to_nhwc(x)
    B, C, H, W = x.shape
    assert C % 4 == 0
    out, ldy = empty_nhwc(B, 4 * C, H, W, x.device)
    t0 = TIMER.start() if TIMER else None
    code = _lib.lib().mydet_spp_concat_f32(_ptr(x), ldx, _ptr(out), ldy, B, H, W, C, int(ks[0]), int(ks[1]), int(ks[2]), _stream())
    if t0:
        TIMER.stop('spp_concat', t0, *[4.0 * B * H * W * C * 5] * 2)
    _lib.check(code, 'mydet_spp_concat_f32')
    return out


def _box_width(mode):
    """Floats per candidate box written by a decode mode: (cx, cy, w, h), or (cx, cy, w, h, deg) for RAPiD."""
    return 5 if mode == DECODE_RAPID else 4


def decode(mode, box, ldbox, box_astride, box_c0, cls, ldcls, cls_astride, cls_c0, conf_c0, anchors_wh, A, C,
           B, H, W, stride, img_hw, bbox, class_idx, score, n_off):
    """Decode one level into bbox[B,N,4] ([B,N,5] for DECODE_RAPID) / class_idx[B,N] / score[B,N] at candidate offset
    n_off."""
    require_gpu(box, 'decode')
    assert bbox.shape[-1] == _box_width(mode) and bbox.is_contiguous()
    N = bbox.shape[1]
    anch = None
    if anchors_wh is not None:
        anch = np.ascontiguousarray(np.asarray(anchors_wh, dtype=np.float32).reshape(-1))
        assert anch.size == 2 * A
    t0 = TIMER.start() if TIMER else None
    code = _lib.lib().mydet_decode_f32(
        mode, _ptr(box), ldbox, box_astride, box_c0, _ptr(cls), ldcls, cls_astride, cls_c0, conf_c0,
        ctypes.c_void_p(anch.ctypes.data) if anch is not None else ctypes.c_void_p(0), A, C, B, H, W,
        float(stride), int(img_hw[0]), int(img_hw[1]), _ptr(bbox), _ptr(class_idx), _ptr(score), N, n_off,
        _stream())
    if t0:      # algorithmic bytes: every head logit once + 28 B per candidate (32 B for RAPiD's 5-float rows)
        per_pix = A * (C + _box_width(mode) + (0 if mode == DECODE_RETINA else 1))
        TIMER.stop('decode', t0, *[4.0 * B * H * W * per_pix + (12.0 + 4 * _box_width(mode)) * B * A * H * W] * 2)
    _lib.check(code, 'mydet_decode_f32')


def _decode_levels(entry, head, mode, levels, box_astride, box_c0, cls_astride, cls_c0, conf_c0, A, C, B, img_hw, bbox,
                   class_idx, score):
    """The level table, timer span and call shared by the multi-level decode entry points: `entry` is the C symbol, `head`
    its arguments in front of the level count ((mode,) or ()), `mode` the decode whose bytes are accounted."""
    require_gpu(bbox, 'decode_levels')
    assert bbox.shape[-1] == _box_width(mode) and bbox.is_contiguous()
    n = len(levels)
    arr = (_lib.DecodeLevel * n)()
    keep = []                                         # host anchor arrays must outlive the call
    work = 0.0
    for i, lv in enumerate(levels):
        anch = None
        if lv['anchors_wh'] is not None:
            anch = np.ascontiguousarray(np.asarray(lv['anchors_wh'], dtype=np.float32).reshape(-1))
            assert anch.size == 2 * A
            keep.append(anch)
        arr[i] = _lib.DecodeLevel(lv['box'].data_ptr(), lv['ldbox'], lv['cls'].data_ptr(), lv['ldcls'],
                                  anch.ctypes.data if anch is not None else None, lv['H'], lv['W'], float(lv['stride']),
                                  lv['n_off'])
        per_pix = A * (C + _box_width(mode) + (0 if mode == DECODE_RETINA else 1))
        work += 4.0 * B * lv['H'] * lv['W'] * per_pix + (12.0 + 4 * _box_width(mode)) * B * A * lv['H'] * lv['W']
    t0 = TIMER.start() if TIMER else None
    code = getattr(_lib.lib(), entry)(*head, n, ctypes.cast(arr, ctypes.c_void_p), box_astride, box_c0, cls_astride, cls_c0,
                                      conf_c0, A, C, B, int(img_hw[0]), int(img_hw[1]), _ptr(bbox), _ptr(class_idx),
                                      _ptr(score), bbox.shape[1], _stream())
    if t0:
        TIMER.stop('decode', t0, work, work)
    _lib.check(code, entry)


def decode_levels(mode, levels, box_astride, box_c0, cls_astride, cls_c0, conf_c0, A, C, B, img_hw, bbox, class_idx,
                  score):
    """Decode every pyramid level with one launch.  levels: list of dicts with keys box, ldbox, cls, ldcls,
    anchors_wh (array-like [A,2] or None), H, W, stride, n_off."""
    _decode_levels('mydet_decode_levels_f32', (mode,), mode, levels, box_astride, box_c0, cls_astride, cls_c0, conf_c0, A, C,
                   B, img_hw, bbox, class_idx, score)


def decode_uv5_levels(levels, box_astride, box_c0, cls_astride, cls_c0, conf_c0, A, C, B, img_hw, bbox, class_idx, score):
    """The Ultralytics (YOLOv5) decode of every pyramid level with one launch (mydet_decode_uv5_levels_f32): arguments as
    decode_levels without the mode; the head layout, bytes and outputs are DECODE_YOLO's."""
    _decode_levels('mydet_decode_uv5_levels_f32', (), DECODE_YOLO, levels, box_astride, box_c0, cls_astride, cls_c0, conf_c0,
                   A, C, B, img_hw, bbox, class_idx, score)


def decode_uv5(box, ldbox, box_astride, box_c0, cls, ldcls, cls_astride, cls_c0, conf_c0, anchors_wh, A, C, B, H, W, stride,
               img_hw, bbox, class_idx, score, n_off):
    """The Ultralytics decode of one level into bbox[B,N,4] / class_idx[B,N] / score[B,N] at candidate offset n_off."""
    require_gpu(box, 'decode_uv5')
    level = dict(box=box, ldbox=ldbox, cls=cls, ldcls=ldcls, anchors_wh=anchors_wh, H=H, W=W, stride=stride, n_off=n_off)
    decode_uv5_levels([level], box_astride, box_c0, cls_astride, cls_c0, conf_c0, A, C, B, img_hw, bbox, class_idx, score)


def record_words(box_width):
    """int32 words of one detection record for candidate boxes of `box_width` floats: REC_WORDS (cxcywh) or
    REC_ROT_WORDS (cxcywhd: the same record + the angle plane)."""
    if box_width not in (4, 5):
        raise ValueError(f'detection records hold boxes of 4 or 5 floats, not {box_width}')
    return _lib.REC_WORDS if box_width == 4 else _lib.REC_ROT_WORDS


def record_views(records):
    """Field views of a detection-record buffer (int32 [B, REC_WORDS], or [B, REC_ROT_WORDS] for rotated boxes;
    include/mydet.h MYDET_REC_*): nothing is copied -- the dict the rest of the package works with IS the wire buffer of
    the multi-GPU exchange.  A rotated record adds 'angle' [B,512]; 'bbox' stays the [B,512,4] plane (cx, cy, w, h)."""
    B = records.shape[0]
    assert records.dtype == torch.int32 and records.shape[1] in (_lib.REC_WORDS, _lib.REC_ROT_WORDS) and records.is_contiguous()
    k = _lib.REC_TOPK
    out = {'count': records[:, _lib.REC_COUNT],
           'bbox': records[:, _lib.REC_BBOX:_lib.REC_SCORE].view(torch.float32).view(B, k, 4),
           'score': records[:, _lib.REC_SCORE:_lib.REC_CLASS].view(torch.float32),
           'class_idx': records[:, _lib.REC_CLASS:_lib.REC_INDEX].view(torch.int64),
           'index': records[:, _lib.REC_INDEX:_lib.REC_WORDS],
           'records': records}
    if records.shape[1] == _lib.REC_ROT_WORDS:
        out['angle'] = records[:, _lib.REC_ANGLE:_lib.REC_ROT_WORDS].view(torch.float32)
    return out


def _record_buffer(what, rec):
    """The 'records' buffer of a record dict (record_views), checked: int32 [B, REC_WORDS | REC_ROT_WORDS] with packed words,
    and the dict's fields views of it -- a graph replay hands out copies, which say nothing about the buffer a launch reads."""
    if not isinstance(rec, dict) or 'records' not in rec or 'bbox' not in rec:
        raise TypeError(f'{what}: rec is the dict of ops.record_views, got {type(rec).__name__}')
    records = rec['records']
    if not isinstance(records, torch.Tensor) or records.dtype != torch.int32 or records.dim() != 2 or \
            records.shape[1] not in (_lib.REC_WORDS, _lib.REC_ROT_WORDS) or records.stride(1) != 1 or records.stride(0) < 0:
        raise ValueError(f'{what}: int32 records [B, {_lib.REC_WORDS} | {_lib.REC_ROT_WORDS}] expected')
    if rec['bbox'].data_ptr() != records.data_ptr() + 4 * _lib.REC_BBOX:
        raise ValueError(f"{what}: the fields of this record dict are copies, not views of its 'records' buffer")
    return records


def record_boxes(rec, b, k):
    """The first k boxes of image b of a record dict as [k, 4] (cxcywh) or [k, 5] (cxcywhd: the angle column appended)."""
    if 'angle' not in rec:
        return rec['bbox'][b, :k]
    return torch.cat([rec['bbox'][b, :k], rec['angle'][b, :k, None]], dim=1)


def _rot_entry(width, rotated_nms, plain, rot, rotnms):
    """Entry point for boxes of `width` floats; `rotated_nms` (cxcywhd only) selects the rotated-IoU NMS."""
    if rotated_nms and width != 5:
        raise ValueError(f"rotated_nms needs 'cxcywhd' boxes (5 floats per row), not rows of {width}")
    return plain if width == 4 else (rotnms if rotated_nms else rot)


NMS_KINDS = {'hard': _lib.NMS_HARD, 'soft-linear': _lib.NMS_SOFT_LINEAR, 'soft-gaussian': _lib.NMS_SOFT_GAUSSIAN,
             'merge': _lib.NMS_MERGE}                                      # MYDET_NMS_* of include/mydet.h


class Nms:
    """How the post-process suppresses, the `nms=` argument of ops.postprocess, ImageObjects.post_process and the Detector
    methods (include/mydet.h, "NMS modes", has the rules the kernel is held to).  kind: 'hard' (greedy, the default),
    'soft-linear' or 'soft-gaussian' (Soft-NMS, Bodla et al. 2017: overlapped boxes lose score instead of being removed; the
    output scores are the decayed ones) or 'merge' (hard NMS, then every kept box becomes the score-weighted mean of the
    boxes it suppressed and itself).  agnostic: all classes are one group -- two classes on one box leave one box.  sigma:
    the width of the Gaussian decay exp(-iou^2 / sigma).  min_score: a soft kind stops emitting a group at the first score
    below it; None = the call's conf_thres.  Immutable; compares and hashes by value.  Touches no device."""
    __slots__ = ('kind', 'agnostic', 'sigma', 'min_score')

    def __init__(self, kind='hard', agnostic=False, sigma=0.5, min_score=None):
        if not isinstance(kind, str) or kind not in NMS_KINDS:
            raise ValueError(f'Nms: kind {kind!r} is not one of {sorted(NMS_KINDS)}')
        if not isinstance(agnostic, (bool, int)) or agnostic not in (0, 1):
            raise ValueError(f'Nms: agnostic is True or False, got {agnostic!r}')
        try:
            sigma = float(sigma)
            min_score = None if min_score is None else float(min_score)
        except (TypeError, ValueError):
            raise ValueError(f'Nms: sigma and min_score are numbers, got {sigma!r} and {min_score!r}') from None
        if not (0 < sigma < math.inf):
            raise ValueError(f'Nms: sigma {sigma!r} is not a finite number above 0')
        if min_score is not None and not (0 <= min_score < math.inf):
            raise ValueError(f'Nms: min_score {min_score!r} is not a finite number >= 0 (or None: the conf_thres of the call)')
        for name, v in zip(self.__slots__, (kind, bool(agnostic), sigma, min_score)):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError('Nms is immutable')

    def _key(self):
        return (self.kind, self.agnostic, self.sigma, self.min_score)

    def __eq__(self, other):
        return isinstance(other, Nms) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return f'Nms({self.kind!r}, agnostic={self.agnostic}, sigma={self.sigma}, min_score={self.min_score})'

    @property
    def plain(self):
        """The class-aware hard NMS: what a call without `nms=` runs."""
        return self.kind == 'hard' and not self.agnostic


def nms_mode(what, nms, conf_thres, box_width, rotated_nms=False):
    """The _lib.NmsMode of an `nms=` argument for candidates of `box_width` floats, or None for today's call (nms None, or
    the plain hard NMS together with rotated_nms).  Raises for what the library has no kernel for or rejects -- a TypeError
    for anything but an Nms, a ValueError otherwise -- before any device is touched."""
    if nms is None:
        return None
    if not isinstance(nms, Nms):
        raise TypeError(f'{what}: nms is a mydetection_amd.api.Nms (or None), got {type(nms).__name__}')
    if rotated_nms:
        if nms.plain:
            return None
        raise ValueError(f'{what}: rotated_nms compares rotated rectangles under the class-aware hard NMS only, not with {nms!r}')
    conf = float(conf_thres)
    if nms.kind == 'merge':
        if box_width != 4:
            raise ValueError(f"{what}: Nms('merge') needs 'cxcywh' boxes; a mean of the angles of 'cxcywhd' boxes is not defined")
        if not conf > 0:
            raise ValueError(f"{what}: Nms('merge') weighs boxes by their scores and needs conf_thres > 0, got {conf_thres!r}")
    if nms.kind in ('soft-linear', 'soft-gaussian') and not conf >= 0:
        raise ValueError(f'{what}: Nms({nms.kind!r}) decays scores towards 0 and needs conf_thres >= 0, got {conf_thres!r}')
    min_score = conf if nms.min_score is None else nms.min_score
    return _lib.NmsMode(NMS_KINDS[nms.kind], int(nms.agnostic), nms.sigma, min_score, 0)


def postprocess(bbox, class_idx, score, conf_thres, nms_thres, topk=TOPK, records=None, rotated_nms=False, nms=None):
    """Batched filter/top-k/class-aware NMS.  bbox [B,N,4], class_idx [B,N] i64, score [B,N].  bbox [B,N,5]
    (cxcywhd) takes the rotated kernel: the same decisions on columns 0-3, rotated records ('angle' added).
    rotated_nms=True (cxcywhd only, ValueError otherwise): the NMS compares the rotated rectangles -- exact intersection
    area, suppress at IoU >= nms_thres (include/mydet.h: mydet_postprocess_records_rotnms_f32); same records.

    Returns dict of device tensors: count [B] i32, bbox [B,512,4], class_idx [B,512] i64, score [B,512],
    index [B,512] i32 -- all views of 'records' (int32 [B, REC_WORDS]), which the kernel writes directly in the
    wire layout of the all-gather (parallel.gather_detections).  Class ids must lie in [0, 4096): an image whose
    selected candidates break that gets count = -1 (`check_counts` raises on it) instead of aliased classes.
    nms: None, or an Nms -- class-agnostic suppression, Soft-NMS or box merging in the same launch (include/mydet.h, "NMS
    modes": the mydet_postprocess_records_*nms_f32 entry points); not with rotated_nms (ValueError).
    """
    fn = _rot_entry(bbox.shape[-1], rotated_nms, 'mydet_postprocess_records_f32', 'mydet_postprocess_records_rot_f32',
                    'mydet_postprocess_records_rotnms_f32')
    mode = nms_mode('postprocess', nms, conf_thres, bbox.shape[-1], rotated_nms)
    if mode is not None:
        fn = 'mydet_postprocess_records_nms_f32' if bbox.shape[-1] == 4 else 'mydet_postprocess_records_rot_nms_f32'
    require_gpu(bbox, 'postprocess')
    assert bbox.dtype == torch.float32 and score.dtype == torch.float32 and class_idx.dtype == torch.int64
    assert topk == TOPK
    bbox, class_idx, score = bbox.contiguous(), class_idx.contiguous(), score.contiguous()
    B, N = score.shape
    dev = bbox.device
    words = record_words(bbox.shape[-1])
    if records is None:
        records = torch.empty((B, words), dtype=torch.int32, device=dev)
    assert records.dtype == torch.int32 and tuple(records.shape) == (B, words) and records.is_contiguous()
    scratch = torch.empty((B, max(N, 1)), dtype=torch.int64, device=dev)
    t0 = TIMER.start() if TIMER else None
    args = (_ptr(bbox), _ptr(class_idx), _ptr(score), B, N, float(conf_thres), float(nms_thres))
    code = getattr(_lib.lib(), fn)(*args, *(() if mode is None else (ctypes.byref(mode),)), _ptr(records), _ptr(scratch), _stream())
    if t0:
        TIMER.stop('postprocess', t0, float(B))
    _lib.check(code, fn)
    return record_views(records)


def postprocess_dense(bbox, class_idx, score, conf_thres, nms_thres, topk=TOPK, rotated_nms=False, nms=None):
    """The same filter/top-k/NMS into dense per-image arrays (mydet_postprocess_f32, or mydet_postprocess_rot_f32 for
    bbox [B,N,5], mydet_postprocess_rotnms_f32 with rotated_nms): count [B] i32, bbox [B,topk,4 or 5], class_idx [B,topk] i64,
    score [B,topk], index [B,topk] i32.  nms: as in postprocess (mydet_postprocess_nms_f32 / mydet_postprocess_rot_nms_f32)."""
    fn = _rot_entry(bbox.shape[-1], rotated_nms, 'mydet_postprocess_f32', 'mydet_postprocess_rot_f32', 'mydet_postprocess_rotnms_f32')
    mode = nms_mode('postprocess_dense', nms, conf_thres, bbox.shape[-1], rotated_nms)
    if mode is not None:
        fn = 'mydet_postprocess_nms_f32' if bbox.shape[-1] == 4 else 'mydet_postprocess_rot_nms_f32'
    require_gpu(bbox, 'postprocess_dense')
    assert bbox.dtype == torch.float32 and score.dtype == torch.float32 and class_idx.dtype == torch.int64
    bbox, class_idx, score = bbox.contiguous(), class_idx.contiguous(), score.contiguous()
    B, N = score.shape
    width = bbox.shape[-1]
    record_words(width)
    dev = bbox.device
    out = {'count': torch.empty(B, dtype=torch.int32, device=dev),
           'bbox': torch.empty((B, topk, width), dtype=torch.float32, device=dev),
           'class_idx': torch.empty((B, topk), dtype=torch.int64, device=dev),
           'score': torch.empty((B, topk), dtype=torch.float32, device=dev),
           'index': torch.empty((B, topk), dtype=torch.int32, device=dev)}
    scratch = torch.empty((B, max(N, 1)), dtype=torch.int64, device=dev)
    args = (_ptr(bbox), _ptr(class_idx), _ptr(score), B, N, float(conf_thres), float(nms_thres), int(topk))
    code = getattr(_lib.lib(), fn)(*args, *(() if mode is None else (ctypes.byref(mode),)), _ptr(out['count']), _ptr(out['bbox']),
                                   _ptr(out['class_idx']), _ptr(out['score']), _ptr(out['index']), _ptr(scratch), _stream())
    _lib.check(code, fn)
    return out


def check_counts(counts):
    """Raise on the kernel's error sentinel in a host copy of the per-image counts (include/mydet.h:
    MYDET_COUNT_BAD_CLASS)."""
    bad = [b for b, k in enumerate(counts) if k < 0]
    if bad:
        raise ValueError(f'postprocess: class ids outside [0, 4096) among the selected candidates of image(s) {bad}; '
                         'the class-aware NMS key holds 12 class bits')
    return counts


def tile_windows(H, W, size, overlap=0.2, full_frame=True, align=1):
    """The windows (y0, x0, h, w) of tiled detection on an H x W frame, as a list.  Host arithmetic only.
    size = (th, tw) (or one int), clipped to the frame: every tile is h = min(th, H) by w = min(tw, W).  Per axis the step is
    max(align, floor(h * (1 - overlap)) // align * align); origins are 0, step, 2*step, ... while origin + h < H, then H - h
    (the last tile ends at the frame's edge), duplicates dropped.  Row-major by (y0, x0).  With full_frame and more than one
    tile the window (0, 0, H, W) follows last.  align=2 is for 4:2:0 planes: H, W, h, w must be even, every origin then is,
    and a window of the planes is itself a 4:2:0 frame.  ValueError for an overlap outside [0, 1), a non-positive size, a
    size that breaks the alignment, or more than _lib.TILES_MAX windows."""
    th, tw = (size, size) if isinstance(size, int) else size
    H, W, th, tw, align = int(H), int(W), int(th), int(tw), int(align)
    if min(H, W) < 1 or min(th, tw) < 1 or align < 1:
        raise ValueError(f'tile_windows: positive sizes expected, got a {H}x{W} frame, tiles {th}x{tw}, align {align}')
    if not 0 <= overlap < 1:
        raise ValueError(f'tile_windows: overlap {overlap!r} is outside [0, 1)')
    h, w = min(th, H), min(tw, W)
    if any(v % align for v in (H, W, h, w)):
        raise ValueError(f'tile_windows: align={align} needs frame and tile sizes that are multiples of it, got a {H}x{W} frame '
                         f'and {h}x{w} tiles')

    def origins(n, t):
        step = max(align, math.floor(t * (1 - overlap)) // align * align)
        return list(range(0, n - t, step)) + [n - t]                 # origin + t < n, then the tile that ends at the edge
    windows = [(y0, x0, h, w) for y0 in origins(H, h) for x0 in origins(W, w)]
    if full_frame and len(windows) > 1:
        windows.append((0, 0, H, W))
    if len(windows) > _lib.TILES_MAX:
        raise ValueError(f'tile_windows: {len(windows)} windows of {h}x{w} on a {H}x{W} frame; at most {_lib.TILES_MAX} are merged')
    return windows


MERGE_METRICS = {'iou': _lib.MERGE_IOU, 'ios': _lib.MERGE_IOS}          # MYDET_MERGE_* of include/mydet.h


def merge_metric_id(metric):
    """The C selector of a pair-test name; a ValueError for an unknown one (raised before any device is touched)."""
    if not isinstance(metric, str) or metric not in MERGE_METRICS:
        raise ValueError(f'merge_tile_records: metric {metric!r} is not one of {sorted(MERGE_METRICS)}')
    return MERGE_METRICS[metric]


def merge_tile_records(rec, B, T, origins, nms_thres, metric='iou', rotated_nms=False, records=None, agnostic=False):
    """The records of T windows of each of B frames -> B records in frame coordinates, by one more class-aware NMS on the
    device (include/mydet.h: mydet_merge_tile_records_f32, where the candidate order, the tie rule and the pair tests are).
    rec: the window records, boxes in window pixel coordinates -- an int32 tensor [T*B, words] (tile-major: window t of
    frame b in row t*B + b) or [T, B, words] with any strides along T and B (a frame-major buffer is
    buf.view(B, T, words).transpose(0, 1)), or the record_views dict of such a [T*B, words] buffer.  origins: T pairs
    (x0, y0), or an int32 device tensor [T, 2].  metric: 'iou' or 'ios' (intersection over the smaller area); rotated_nms:
    the rotated-IoU test (rotated records and 'iou' only).  records: optional int32 [B, words] buffer to write.  agnostic:
    the merge's NMS has one group of all classes (mydet_merge_tile_records_nms_f32; both metrics, not with rotated_nms).
    Returns the record_views dict of the merged records; 'index' holds t*512 + k of every survivor."""
    m = merge_metric_id(metric)
    if agnostic and rotated_nms:
        raise ValueError('merge_tile_records: agnostic is defined for the axis-aligned tests only, not with rotated_nms')
    if isinstance(rec, dict):
        rec = _record_buffer('merge_tile_records', rec)
    require_gpu(rec, 'merge_tile_records')
    B, T = int(B), int(T)
    words = rec.shape[-1]
    if rec.dtype != torch.int32 or words not in (_lib.REC_WORDS, _lib.REC_ROT_WORDS):
        raise ValueError(f'merge_tile_records: int32 records of {_lib.REC_WORDS} or {_lib.REC_ROT_WORDS} words expected, got '
                         f'{rec.dtype} {tuple(rec.shape)}')
    width = 4 if words == _lib.REC_WORDS else 5
    if rotated_nms and width != 5:
        raise ValueError("rotated_nms needs 'cxcywhd' records (the rotated record with its angle plane)")
    if rotated_nms and m == _lib.MERGE_IOS:
        raise ValueError("merge_tile_records: metric 'ios' is defined for the axis-aligned test only, not with rotated_nms")
    if not 1 <= T <= _lib.TILES_MAX or B < 1:
        raise ValueError(f'merge_tile_records: B >= 1 and 1 <= T <= {_lib.TILES_MAX} expected, got B = {B}, T = {T}')
    if rec.dim() == 2:
        rec = rec.contiguous().view(T, B, words) if rec.shape[0] == T * B else rec
    if tuple(rec.shape) != (T, B, words):
        raise ValueError(f'merge_tile_records: records of shape [{T * B}, {words}] or [{T}, {B}, {words}] expected, got {tuple(rec.shape)}')
    if rec.stride(2) != 1 or rec.stride(0) % 4 or rec.stride(1) % 4 or min(rec.stride(0), rec.stride(1)) < 0:
        rec = rec.contiguous()
    dev = rec.device
    if isinstance(origins, torch.Tensor):
        org = origins
    else:
        org = torch.tensor([[int(x0), int(y0)] for x0, y0 in origins], dtype=torch.int32).reshape(-1, 2).to(dev, non_blocking=True)
    if org.dtype != torch.int32 or tuple(org.shape) != (T, 2) or org.device != dev or not org.is_contiguous():
        raise ValueError(f'merge_tile_records: {T} origins (x0, y0) expected (an int32 tensor [{T}, 2] on {dev}), got {tuple(org.shape)}')
    if records is None:
        records = torch.empty((B, words), dtype=torch.int32, device=dev)
    assert records.dtype == torch.int32 and tuple(records.shape) == (B, words) and records.is_contiguous() and records.device == dev
    nbytes = _lib.lib().mydet_merge_tile_records_scratch_bytes(B, T, width)
    scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    t0 = TIMER.start() if TIMER else None
    head = (_ptr(rec), rec.stride(0), rec.stride(1), B, T, width, _ptr(org), float(nms_thres), m, int(bool(rotated_nms)))
    fn = 'mydet_merge_tile_records_nms_f32' if agnostic else 'mydet_merge_tile_records_f32'
    code = getattr(_lib.lib(), fn)(*head, *((1,) if agnostic else ()), _ptr(records), _ptr(scratch), nbytes, _stream())
    if t0:
        TIMER.stop('merge_tile_records', t0, float(B))
    _lib.check(code, fn)
    return record_views(records)


FUSE_KINDS = {'nms': _lib.FUSE_NMS, 'wbf': _lib.FUSE_WBF}              # MYDET_FUSE_* of include/mydet.h
VIEWS_MAX = _lib.VIEWS_MAX


def fuse_view_records(rec, B, V, flips, frame_hw, thres, kind='nms', metric='iou', rotated_nms=False, agnostic=False, min_score=0.0,
                      records=None):
    """The records of V mirrored views of each of B frames -> B records in frame coordinates: test-time augmentation
    (include/mydet.h: mydet_fuse_view_records_f32, where the view transform, the candidate order and the WBF rules are).
    rec: the view records, boxes in the pixel coordinates of the mirrored frame -- an int32 tensor [V*B, words] (view-major: view
    v of frame b in row v*B + b) or [V, B, words] with any strides along V and B, or the record_views dict of a [V*B, words]
    buffer.  flips: V views, each 0..3 or '', 'h', 'v', 'hv' (view_flip_bits).  frame_hw: (H, W) of the frames.  kind: 'nms' --
    merge_tile_records at zero origins after the view transform, with its metric / rotated_nms / agnostic -- or 'wbf', Weighted
    Boxes Fusion ('cxcywh' records, 'iou', no rotated_nms; clusters whose fused score is below min_score are dropped).  thres: the
    overlap above which two boxes are one object.  records: optional int32 [B, words] buffer to write.  Every argument error
    is a ValueError raised before any device is touched.  Returns the record_views dict; 'index' holds v*512 + k of a survivor
    (kind 'nms') or of a cluster's first member ('wbf')."""
    what = 'fuse_view_records'
    if not isinstance(kind, str) or kind not in FUSE_KINDS:
        raise ValueError(f'{what}: kind {kind!r} is not one of {sorted(FUSE_KINDS)}')
    if not isinstance(metric, str) or metric not in MERGE_METRICS:
        raise ValueError(f'{what}: metric {metric!r} is not one of {sorted(MERGE_METRICS)}')
    m = MERGE_METRICS[metric]
    B, V = int(B), int(V)
    if not 1 <= V <= _lib.VIEWS_MAX or B < 1:
        raise ValueError(f'{what}: B >= 1 and 1 <= V <= {_lib.VIEWS_MAX} expected, got B = {B}, V = {V}')
    flips = [view_flip_bits(f, what) for f in flips]
    if len(flips) != V:
        raise ValueError(f'{what}: {V} flips expected, got {len(flips)}')
    H, W = int(frame_hw[0]), int(frame_hw[1])
    if H < 1 or W < 1:
        raise ValueError(f'{what}: a positive frame size expected, got {H}x{W}')
    min_score = float(min_score)
    if not min_score >= 0.0:
        raise ValueError(f'{what}: min_score >= 0 expected, got {min_score}')
    if isinstance(rec, dict):
        rec = _record_buffer(what, rec)
    if not isinstance(rec, torch.Tensor) or rec.dtype != torch.int32 or rec.shape[-1] not in (_lib.REC_WORDS, _lib.REC_ROT_WORDS):
        raise ValueError(f'{what}: int32 records of {_lib.REC_WORDS} or {_lib.REC_ROT_WORDS} words expected')
    words = rec.shape[-1]
    width = 4 if words == _lib.REC_WORDS else 5
    if rotated_nms and width != 5:
        raise ValueError(f"{what}: rotated_nms needs 'cxcywhd' records (the rotated record with its angle plane)")
    if kind == 'wbf':
        if width != 4:
            raise ValueError(f"{what}: kind 'wbf' is defined for 'cxcywh' records only (no mean of angles)")
        if m != _lib.MERGE_IOU or rotated_nms:
            raise ValueError(f"{what}: kind 'wbf' takes metric 'iou' and no rotated_nms")
    elif rotated_nms and (m == _lib.MERGE_IOS or agnostic):
        raise ValueError(f"{what}: rotated_nms goes with metric 'iou' and without agnostic")
    if rec.dim() == 2 and rec.shape[0] == V * B:
        rec = rec.contiguous().view(V, B, words)
    if tuple(rec.shape) != (V, B, words):
        raise ValueError(f'{what}: records of shape [{V * B}, {words}] or [{V}, {B}, {words}] expected, got {tuple(rec.shape)}')
    require_gpu(rec, what)
    if rec.stride(2) != 1 or rec.stride(0) % 4 or rec.stride(1) % 4 or min(rec.stride(0), rec.stride(1)) < 0:
        rec = rec.contiguous()
    dev = rec.device
    if records is None:
        records = torch.empty((B, words), dtype=torch.int32, device=dev)
    assert records.dtype == torch.int32 and tuple(records.shape) == (B, words) and records.is_contiguous() and records.device == dev
    mode = _lib.FuseMode(FUSE_KINDS[kind], m, int(bool(rotated_nms)), int(bool(agnostic)), min_score, 0)
    nbytes = _lib.lib().mydet_fuse_view_records_scratch_bytes(B, V, width, mode.kind)
    scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    host_flips = (ctypes.c_int32 * V)(*flips)
    t0 = TIMER.start() if TIMER else None
    code = _lib.lib().mydet_fuse_view_records_f32(_ptr(rec), rec.stride(0), rec.stride(1), B, V, width, host_flips, H, W, float(thres),
                                                  ctypes.byref(mode), _ptr(records), _ptr(scratch), nbytes, _stream())
    if t0:
        TIMER.stop('fuse_view_records', t0, float(B))
    _lib.check(code, 'mydet_fuse_view_records_f32')
    return record_views(records)


# ---------------------------------------------------------------------------------------------------------------------------
# Per-stream state: the tracker and what sits behind it (zones, trails, camera motion, appearance) each keep an int32
# [streams, words] buffer.  The rules of such a buffer are stated once here; a family is one record of what differs: the name
# of its functions (`<name>_reset_`), the prefix of its messages, words(*args): the row length, what_for: the format of what that
# length belongs to, reset: the C entry that fills the rows (None: zeros) and reset_args(*args): its arguments between the stream
# count and the HIP stream, gpu: whether a host tensor is refused.
_StateFamily = collections.namedtuple('_StateFamily', 'name prefix words what_for reset reset_args gpu')


def check_streams(prefix, streams):
    streams = int(streams)
    if streams < 1:
        raise ValueError(f'{prefix}: streams >= 1 expected, got {streams}')
    return streams


def _max_tracks(prefix, max_tracks):
    max_tracks = int(max_tracks)
    if not 1 <= max_tracks <= _lib.TRACK_MAX_TRACKS:
        raise ValueError(f'{prefix}: 1 <= max_tracks <= {_lib.TRACK_MAX_TRACKS} expected, got {max_tracks}')
    return max_tracks


def _row_slots(state, header, slot_words):
    """max_tracks by the row length of a slot family's state, for the views that take None; 1 for what is no state at all."""
    if not isinstance(state, torch.Tensor) or state.dim() != 2:
        return 1
    return max((state.shape[1] - header) // slot_words, 1)


def _state_check(fam, state, args, what, views=False):
    """The state rule: a contiguous int32 [streams, fam.words(*args)] tensor, on a GPU unless the family or the caller
    (views: the field views work on a host copy) says otherwise."""
    words = fam.words(*args)
    if not isinstance(state, torch.Tensor) or state.dtype != torch.int32 or state.dim() != 2 or state.shape[1] != words or not state.is_contiguous():
        got = f'{state.dtype} {tuple(state.shape)}' if isinstance(state, torch.Tensor) else type(state).__name__
        raise ValueError(f'{what}: a contiguous int32 state [streams, {words} words] for {fam.what_for.format(*args)} expected, got {got}')
    if fam.gpu and not views:
        require_gpu(state, what)


def _state_reset(fam, state, args):
    _state_check(fam, state, args, f'{fam.name}_reset_')
    if fam.reset is None:
        return state.zero_()
    code = getattr(_lib.lib(), fam.reset)(_ptr(state), state.shape[0], *fam.reset_args(*args), _stream())
    _lib.check(code, fam.reset)
    return state


def _state_new(fam, streams, args, device):
    """Allocate [streams, words] and reset it."""
    words = fam.words(*args)                                         # the rules of `args` first, then that of `streams`
    return _state_reset(fam, torch.empty((check_streams(fam.prefix, streams), words), dtype=torch.int32, device=device), args)


def _check_planes(what, name, planes, shapes, dev):
    """The check-only half of out_planes, for a dict that another call made (`name`: what the message calls it)."""
    for k, (shape, dt) in shapes.items():
        t = planes[k]
        if tuple(t.shape) != shape or t.dtype != dt or t.device != dev or not t.is_contiguous():
            raise ValueError(f'{what}: {name}[{k!r}] must be a contiguous {dt} tensor {shape} on {dev}')
    return planes


def out_planes(what, out, shapes, dev):
    """The output dict of a *_frames call.  shapes: name -> (shape, dtype).  out None: allocated on `dev`; else every named entry
    of `out` must be a contiguous tensor of that shape and dtype on `dev` (a ValueError that names the entry), and `out` is returned."""
    if out is None:
        return {k: torch.empty(shape, dtype=dt, device=dev) for k, (shape, dt) in shapes.items()}
    return _check_planes(what, 'out', out, shapes, dev)


def _ints(*args):
    return tuple(int(a) for a in args)


TRACK_MATCHES = {'iou': _lib.TRACK_MATCH_IOU, 'rotated': _lib.TRACK_MATCH_ROTATED}        # MYDET_TRACK_MATCH_* of include/mydet.h
TRACK_ASSIGNS = {'greedy': _lib.TRACK_ASSIGN_GREEDY, 'optimal': _lib.TRACK_ASSIGN_OPTIMAL}   # MYDET_TRACK_ASSIGN_*
# KFTracklet's constants (reference utils/structures.py:457-460): standard deviations; the kernel takes their squares
TRACK_P0 = (0.1, 0.1, 0.1, 0.1, 10, 0.1, 0.1, 0.1, 0.1, 10)
TRACK_Q = (0.049, 0.032, 0.052, 0.097, 13.62, 0.01, 0.01, 0.01, 0.01, 1)
TRACK_R = (0.073, 0.064, 0.124, 0.163, 24.39)


def track_match_id(match):
    """The C selector of a tracker's pair test; a ValueError for an unknown one (raised before any device is touched)."""
    if not isinstance(match, str) or match not in TRACK_MATCHES:
        raise ValueError(f'track_frames: match {match!r} is not one of {sorted(TRACK_MATCHES)}')
    return TRACK_MATCHES[match]


def track_state_words(max_tracks):
    """int32 words of one stream's tracker state (include/mydet.h: mydet_track_state_words); host arithmetic only."""
    return (_lib.TRACK_STATE_HEADER + _lib.TRACK_SLOT_WORDS * _max_tracks('tracker', max_tracks) + 3) // 4 * 4


_TRACK_STATE = _StateFamily('track', 'tracker', track_state_words, 'max_tracks = {}', 'mydet_track_reset', _ints, True)


def track_variances(std, n, what):
    """n standard deviations -> float32 variances (squared in double, rounded once), as the kernel's parameter struct holds them."""
    v = np.asarray(std, dtype=np.float64).reshape(-1)
    if v.shape != (n,) or not np.all(np.isfinite(v)) or np.any(v < 0):
        raise ValueError(f'tracker: {what} = {n} finite, non-negative standard deviations expected, got {std!r}')
    return np.square(v).astype(np.float32)


def track_params(img_hw, match='iou', match_thres=0.3, new_thres=0.3, max_missed=30, momentum=0.8, min_score=0.1, p0=TRACK_P0,
                 q=TRACK_Q, r=TRACK_R):
    """The parameter struct of mydet_track_frames_f32 (a _lib.TrackParams) from the reference's units: p0, q, r are standard
    deviations (KFTracklet's by default).  ValueError for anything out of range; touches no device."""
    m = track_match_id(match)
    max_missed = int(max_missed)
    if max_missed < 1:
        raise ValueError(f'tracker: max_missed >= 1 expected, got {max_missed}')
    if not 0 <= float(momentum) <= 1:
        raise ValueError(f'tracker: momentum in [0, 1] expected, got {momentum!r}')
    h, w = (float(v) for v in img_hw)
    if not (h > 0 and w > 0):
        raise ValueError(f'tracker: a positive frame size (H, W) expected, got {img_hw!r}')
    p = _lib.TrackParams()
    p.p0[:], p.q[:], p.r[:] = track_variances(p0, 10, 'p0').tolist(), track_variances(q, 10, 'q').tolist(), track_variances(r, 5, 'r').tolist()
    p.momentum, p.min_score, p.new_thres, p.match_thres = float(momentum), float(min_score), float(new_thres), float(match_thres)
    p.img_h, p.img_w, p.max_missed, p.match = h, w, max_missed, m
    return p


def track_assoc(assign='greedy', low_thres=None, high_thres=None, low_match_thres=None):
    """The association mode of mydet_track_frames_assoc_f32 (a _lib.TrackAssoc; include/mydet.h has the rules).  assign: 'greedy'
    or 'optimal'.  low_thres: None for one score band; else the second stage is on and high_thres and low_match_thres are
    required (Tracker fills them from the call's conf_thres and its match_thres).  ValueError for anything out of range;
    touches no device."""
    if not isinstance(assign, str) or assign not in TRACK_ASSIGNS:
        raise ValueError(f'tracker: assign {assign!r} is not one of {sorted(TRACK_ASSIGNS)}')
    a = _lib.TrackAssoc()
    a.assign = TRACK_ASSIGNS[assign]
    if low_thres is None:
        if high_thres is not None or low_match_thres is not None:
            raise ValueError('tracker: high_thres and low_match_thres belong to the second stage; set low_thres to turn it on')
        return a
    if high_thres is None or low_match_thres is None:
        raise ValueError('tracker: with low_thres, high_thres and low_match_thres are required')
    low, high, lm = float(low_thres), float(high_thres), float(low_match_thres)
    if not (np.isfinite(low) and np.isfinite(high) and np.isfinite(lm)):
        raise ValueError(f'tracker: finite low_thres, high_thres and low_match_thres expected, got {low_thres!r}, {high_thres!r}, {low_match_thres!r}')
    a.bands, a.high_thres, a.low_thres, a.low_match_thres = 1, high, low, lm
    if not a.low_thres < a.high_thres:                               # as the kernel compares them: in float32
        raise ValueError(f'tracker: low_thres < high_thres expected, got {low_thres!r} and {high_thres!r}')
    return a


def track_state(streams, max_tracks, device):
    """A reset tracker state: int32 [streams, track_state_words(max_tracks)] (include/mydet.h has the layout)."""
    return _state_new(_TRACK_STATE, streams, (max_tracks,), device)


def track_reset_(state, max_tracks):
    """Reset a tracker state in place (mydet_track_reset): no tracks, the next id of every stream is 1."""
    return _state_reset(_TRACK_STATE, state, (max_tracks,))


def track_state_views(state, max_tracks=None):
    """Field views of a tracker state int32 [S, words] (include/mydet.h: mydet_track_frames_f32), nothing copied: a dict of
    x, v, pxx, pxv, pvv float32 [S,5,MT] (rows cx, cy, w, h, angle), score float32 [S,MT], cls, id int64 [S,MT] (id 0 = a free
    slot), missed int32 [S,MT], next_id int64 [S], live int32 [S].  max_tracks: taken from the row length when None.  Works on
    any device (tests read a host copy)."""
    mt = _row_slots(state, _lib.TRACK_STATE_HEADER, _lib.TRACK_SLOT_WORDS) if max_tracks is None else int(max_tracks)
    _state_check(_TRACK_STATE, state, (mt,), 'track_state_views', views=True)
    S, o = state.shape[0], _lib.TRACK_STATE_HEADER
    out = {'next_id': state[:, 0:2].view(torch.int64)[:, 0], 'live': state[:, 2]}
    out['cls'] = state[:, o:o + 2 * mt].view(torch.int64)
    out['id'] = state[:, o + 2 * mt:o + 4 * mt].view(torch.int64)
    o += 4 * mt
    for name in ('x', 'v', 'pxx', 'pxv', 'pvv'):
        out[name] = state[:, o:o + 5 * mt].view(torch.float32).view(S, 5, mt)
        o += 5 * mt
    out['score'] = state[:, o:o + mt].view(torch.float32)
    out['missed'] = state[:, o + mt:o + 2 * mt]
    return out


def track_frames(records, tracker_state, params, frames_per_stream=None, max_tracks=None, out=None, assoc=None, shift=None, appear=None,
                 appear_weight=None, appear_ws=None, warp=None):
    """Advance S streams by F frames each in ONE launch (include/mydet.h: mydet_track_frames_f32, where the rules are).
    records: the detection records in frame coordinates -- an int32 tensor [S*F, words] (frame f of stream s in row s*F + f) or
    [S, F, words] with any strides along S and F that are multiples of 4 words, or the record_views dict of a [S*F, words]
    buffer; words = REC_WORDS (cxcywh) or REC_ROT_WORDS (cxcywhd).  tracker_state: int32 [S, track_state_words(max_tracks)]
    from track_state, updated in place.  params: track_params(...).  frames_per_stream: F for 2-d records (default: rows / S).
    Returns a dict of device tensors: box [S,F,MT,5], score [S,F,MT], cls, id int64 [S,F,MT] (id 0 = a free slot), missed int32
    [S,F,MT] (0 = matched or born in this frame, -1 = a free slot), count int32 [S,F] (live tracks; MYDET_COUNT_BAD_CLASS for
    a bad-class frame, which leaves the state alone), dropped int32 [S,F].  out: such a dict to write into.  assoc: None for the
    greedy single-band association of mydet_track_frames_f32, or a track_assoc(...) (mydet_track_frames_assoc_f32).  shift:
    None, or the camera motion of the same frames -- motion_frames(...)['shift'], int32 [S,F,4] or [S*F,4] on the records'
    device: in a frame with valid == 1 every prediction moves by (dx, dy) before the association
    (mydet_track_frames_motion_f32).  appear: None, or (appear_set(...), desc, appear_state) -- the descriptors of the same
    frames, uint16 [S*F,512,128] or [S,F,512,128] (appear_records, or any 128 bins that sum to at most 512 per row), and the
    int32 [S, words] state of appear_state, updated in place: the gate, the re-identification and the templates of
    mydet_track_frames_appear_f32 (greedy assignment only: a ValueError with assign 'optimal', before any launch).  The dict
    then also holds sim and how, int32 [S,F,MT].  appear_weight: None, or with appear= an int in 0..256 -- the optimal assignment
    on the fused IoU-and-appearance cost of mydet_track_frames_appear_optimal_f32: m = ((256 - weight) * q + weight * (S >> 1)) >> 8.
    It takes an assoc with assign 'optimal' (a greedy one is a ValueError before any launch) and appear_ws, the int32
    [S, appear_ws_words(max_tracks)] tensor of appear_workspace, which afterwards holds S of the last frame's needed pairs at
    [s, d * max_tracks + j].  warp: None, or in the place of shift the similarity model of the same frames --
    motion_frames(...)['warp'] of a set with model 'similarity', int32 [S,F,8] or [S*F,8] on the records' device: in a frame with
    valid == 1 every prediction is moved, turned and scaled about the frame centre (mydet_track_frames_warp_f32 and its
    appearance siblings).  Both shift and warp: a ValueError before any launch."""
    if shift is not None and warp is not None:
        raise ValueError('track_frames: shift and warp are two forms of one camera motion; pass one of them')
    if not isinstance(params, _lib.TrackParams):
        raise TypeError(f'track_frames: params is a _lib.TrackParams (ops.track_params), got {type(params).__name__}')
    if assoc is not None and not isinstance(assoc, _lib.TrackAssoc):
        raise TypeError(f'track_frames: assoc is a _lib.TrackAssoc (ops.track_assoc) or None, got {type(assoc).__name__}')
    if isinstance(records, dict):
        records = _record_buffer('track_frames', records)
    if not isinstance(tracker_state, torch.Tensor) or tracker_state.dim() != 2:
        raise ValueError('track_frames: tracker_state is the int32 [streams, words] tensor of ops.track_state')
    S = tracker_state.shape[0]
    if max_tracks is None:
        max_tracks = (tracker_state.shape[1] - _lib.TRACK_STATE_HEADER) // _lib.TRACK_SLOT_WORDS
    mt = int(max_tracks)
    words = records.shape[-1]
    if records.dtype != torch.int32 or words not in (_lib.REC_WORDS, _lib.REC_ROT_WORDS):
        raise ValueError(f'track_frames: int32 records of {_lib.REC_WORDS} or {_lib.REC_ROT_WORDS} words expected, got '
                         f'{records.dtype} {tuple(records.shape)}')
    width = 4 if words == _lib.REC_WORDS else 5
    if appear is not None:
        if not isinstance(appear, (tuple, list)) or len(appear) != 3 or not isinstance(appear[0], _lib.TrackAppear):
            raise TypeError('track_frames: appear is (ops.appear_set(...), desc, appear_state) or None')
        if appear_weight is None and assoc is not None and assoc.assign != _lib.TRACK_ASSIGN_GREEDY:
            raise ValueError("track_frames: the appearance runs with assign 'greedy' only (the optimal assignment forms its costs on the fly)")
    if appear_weight is None:
        if appear_ws is not None:
            raise ValueError('track_frames: appear_ws is the workspace of the fused cost and goes with appear_weight')
    else:
        if appear is None:
            raise ValueError('track_frames: appear_weight weighs the appearance of appear=(ops.appear_set(...), desc, appear_state)')
        if isinstance(appear_weight, bool) or not isinstance(appear_weight, (int, np.integer)) or not 0 <= int(appear_weight) <= 256:
            raise ValueError(f'track_frames: appear_weight is None or an int in 0..256, got {appear_weight!r}')
        if assoc is None or assoc.assign != _lib.TRACK_ASSIGN_OPTIMAL:
            raise ValueError("track_frames: the fused IoU-and-appearance cost (appear_weight) runs with assign 'optimal' only "
                             '(the greedy walk keeps its IoU-major key)')
    if params.match == _lib.TRACK_MATCH_ROTATED and width != 5:
        raise ValueError("track_frames: match 'rotated' needs 'cxcywhd' records (the rotated record with its angle plane)")
    if records.dim() == 2:
        F = records.shape[0] // S if frames_per_stream is None else int(frames_per_stream)
        if F < 1 or records.shape[0] != S * F:
            raise ValueError(f'track_frames: {records.shape[0]} records are not F frames of each of {S} streams')
        records = records.contiguous().view(S, F, words)
    if records.dim() != 3 or records.shape[0] != S or records.shape[1] < 1:
        raise ValueError(f'track_frames: records of shape [S*F, {words}] or [{S}, F, {words}] expected, got {tuple(records.shape)}')
    F = records.shape[1]
    _state_check(_TRACK_STATE, tracker_state, (mt,), 'track_frames')
    require_gpu(records, 'track_frames')
    if records.device != tracker_state.device:
        raise ValueError(f'track_frames: records on {records.device}, state on {tracker_state.device}')
    if records.stride(2) != 1 or records.stride(0) % 4 or records.stride(1) % 4 or min(records.stride(0), records.stride(1)) < 0:
        records = records.contiguous()
    dev = records.device
    shapes = {'box': ((S, F, mt, 5), torch.float32), 'score': ((S, F, mt), torch.float32), 'cls': ((S, F, mt), torch.int64),
              'id': ((S, F, mt), torch.int64), 'missed': ((S, F, mt), torch.int32), 'count': ((S, F), torch.int32),
              'dropped': ((S, F), torch.int32)}
    if appear is not None:
        shapes.update(sim=((S, F, mt), torch.int32), how=((S, F, mt), torch.int32))
        aset, desc, astate = appear
        if (not isinstance(desc, torch.Tensor) or desc.dtype != torch.uint16 or desc.numel() != S * F * _lib.REC_TOPK * _lib.APPEAR_BINS or
                tuple(desc.shape[-2:]) != (_lib.REC_TOPK, _lib.APPEAR_BINS) or desc.device != dev or not desc.is_contiguous()):
            raise ValueError(f'track_frames: desc must be a contiguous uint16 tensor [{S * F},{_lib.REC_TOPK},{_lib.APPEAR_BINS}] on {dev}')
        _state_check(_APPEAR_STATE, astate, (mt,), 'track_frames')
        if astate.shape[0] != S or astate.device != dev:
            raise ValueError(f'track_frames: the appearance state must be [{S}, words] on {dev}')
        if appear_weight is not None:
            _workspace_check(appear_ws, S, mt, dev, 'track_frames')
    out = out_planes('track_frames', out, shapes, dev)
    if shift is not None:
        if (not isinstance(shift, torch.Tensor) or shift.dtype != torch.int32 or shift.numel() != S * F * 4 or shift.shape[-1] != 4 or
                shift.device != dev or not shift.is_contiguous()):
            raise ValueError(f'track_frames: shift must be a contiguous int32 tensor [{S},{F},4] on {dev} (ops.motion_frames)')
    if warp is not None:
        if (not isinstance(warp, torch.Tensor) or warp.dtype != torch.int32 or warp.numel() != S * F * 8 or warp.shape[-1] != 8 or
                warp.device != dev or not warp.is_contiguous()):
            raise ValueError(f'track_frames: warp must be a contiguous int32 tensor [{S},{F},8] on {dev} (ops.motion_frames)')
    t0 = TIMER.start() if TIMER else None
    args = (_ptr(records), records.stride(0), records.stride(1), S, F, width, ctypes.byref(params), mt, _ptr(tracker_state), _ptr(out['box']),
            _ptr(out['score']), _ptr(out['cls']), _ptr(out['id']), _ptr(out['missed']), _ptr(out['count']), _ptr(out['dropped']))
    if warp is not None and appear is not None and appear_weight is not None:
        name = 'mydet_track_frames_appear_optimal_warp_f32'
        code = _lib.lib().mydet_track_frames_appear_optimal_warp_f32(*args, ctypes.byref(assoc), _ptr(warp), ctypes.byref(aset), _ptr(desc),
                                                                     _ptr(astate), _ptr(out['sim']), _ptr(out['how']), int(appear_weight),
                                                                     _ptr(appear_ws), _stream())
    elif warp is not None and appear is not None:
        name = 'mydet_track_frames_appear_warp_f32'
        code = _lib.lib().mydet_track_frames_appear_warp_f32(*args, ctypes.byref(track_assoc() if assoc is None else assoc), _ptr(warp),
                                                             ctypes.byref(aset), _ptr(desc), _ptr(astate), _ptr(out['sim']), _ptr(out['how']),
                                                             _stream())
    elif warp is not None:
        name = 'mydet_track_frames_warp_f32'
        code = _lib.lib().mydet_track_frames_warp_f32(*args, ctypes.byref(track_assoc() if assoc is None else assoc), _ptr(warp), _stream())
    elif appear is not None and appear_weight is not None:
        name = 'mydet_track_frames_appear_optimal_f32'
        code = _lib.lib().mydet_track_frames_appear_optimal_f32(*args, ctypes.byref(assoc), None if shift is None else _ptr(shift),
                                                                ctypes.byref(aset), _ptr(desc), _ptr(astate), _ptr(out['sim']),
                                                                _ptr(out['how']), int(appear_weight), _ptr(appear_ws), _stream())
    elif appear is not None:
        name = 'mydet_track_frames_appear_f32'
        code = _lib.lib().mydet_track_frames_appear_f32(*args, ctypes.byref(track_assoc() if assoc is None else assoc),
                                                        None if shift is None else _ptr(shift), ctypes.byref(aset), _ptr(desc), _ptr(astate),
                                                        _ptr(out['sim']), _ptr(out['how']), _stream())
    elif shift is not None:
        name = 'mydet_track_frames_motion_f32'
        code = _lib.lib().mydet_track_frames_motion_f32(*args, ctypes.byref(track_assoc() if assoc is None else assoc), _ptr(shift), _stream())
    elif assoc is None:
        name = 'mydet_track_frames_f32'
        code = _lib.lib().mydet_track_frames_f32(*args, _stream())
    else:
        name = 'mydet_track_frames_assoc_f32'
        code = _lib.lib().mydet_track_frames_assoc_f32(*args, ctypes.byref(assoc), _stream())
    if t0:
        TIMER.stop('track_frames', t0, float(S * F))
    _lib.check(code, name)
    return out


ZONE_ANCHORS = {'center': _lib.ZONE_ANCHOR_CENTER, 'bottom': _lib.ZONE_ANCHOR_BOTTOM}


def zone_quantise(v):
    """q(v) of include/mydet.h (mydet_zones_frames) in numpy float32: 1/16 pixel, floor, clamped to +-2^20."""
    v = np.asarray(v, dtype=np.float32)
    lo, hi = np.float32(-_lib.ZONE_COORD_MAX), np.float32(_lib.ZONE_COORD_MAX)
    return np.floor(np.minimum(np.maximum(v * np.float32(16.0), lo), hi)).astype(np.int32)


def _zone_points(what, pts, n_lo, n_hi):
    try:
        with np.errstate(over='ignore'):                             # too large for float32: an infinity, refused below
            a = np.asarray(pts, dtype=np.float32)
    except (TypeError, ValueError):
        a = None
    if a is None or a.ndim != 2 or a.shape[1] != 2 or not n_lo <= a.shape[0] <= n_hi:
        raise ValueError(f'zone_set: {what} is {n_lo} .. {n_hi} points (x, y), got {pts!r}' if n_lo != n_hi else
                         f'zone_set: {what} is {n_lo} points (x, y), got {pts!r}')
    if not np.all(np.isfinite(a)):
        raise ValueError(f'zone_set: {what} has a non-finite coordinate: {pts!r}')
    return zone_quantise(a)


def _zone_anchor(what, anchor):
    """The C selector of the tested point of a box, 'center' or 'bottom'."""
    if not isinstance(anchor, str) or anchor not in ZONE_ANCHORS:
        raise ValueError(f'{what}: anchor {anchor!r} is not one of {sorted(ZONE_ANCHORS)}')
    return ZONE_ANCHORS[anchor]


def _set_classes(what, struct, classes):
    """classes (None, or 1 .. 16 class indices) into the n_classes and classes fields of a ZoneSet or TrailSet."""
    if classes is None:
        return
    cl = [int(c) for c in classes]
    if not 1 <= len(cl) <= _lib.ZONE_MAX_CLASSES or any(c < 0 or c >= 1 << 31 for c in cl):
        raise ValueError(f'{what}: classes is None or 1 .. {_lib.ZONE_MAX_CLASSES} class indices, got {classes!r}')
    struct.n_classes = len(cl)
    struct.classes[:len(cl)] = cl


def _frame_hw(what, hw):
    """A frame size (H, W) as two integers of 1 .. ZONE_MAX_FRAME each."""
    try:
        h, w = (int(v) for v in hw)
    except (TypeError, ValueError):
        raise ValueError(f'{what}: a frame size (H, W) expected, got {hw!r}') from None
    if not (1 <= h <= _lib.ZONE_MAX_FRAME and 1 <= w <= _lib.ZONE_MAX_FRAME):
        raise ValueError(f'{what}: a frame size (H, W) of 1 .. {_lib.ZONE_MAX_FRAME} each expected, got {hw!r}')
    return h, w


def zone_set(img_hw, polygons=(), lines=(), anchor='center', classes=None, coasting=False, heat=None):
    """The parameter struct of mydet_zones_frames (a _lib.ZoneSet; include/mydet.h has the rules).  img_hw: the frame size
    (H, W), each 1 .. 32768.  polygons: at most 16 sequences of 3 .. 16 points (x, y) in frame pixels; lines: at most 16 pairs
    ((ax, ay), (bx, by)), directed A -> B.  Coordinates are quantised to 1/16 pixel here, by the formula the kernel applies to
    the anchors.  anchor: 'center' (cx, cy) or 'bottom' (cx, cy + h/2).  classes: None, or 1 .. 16 class indices to count.
    coasting: also observe live tracks without a detection in the frame, at their predicted boxes.  heat: None, or (gh, gw),
    each 1 .. 1024.  ValueError for anything out of range, a polygon of zero area or a line of zero length after quantisation,
    non-finite coordinates, or neither polygons nor lines; touches no device."""
    anchor = _zone_anchor('zone_set', anchor)
    h, w = _frame_hw('zone_set', img_hw)
    polygons, lines = list(polygons), list(lines)
    if not polygons and not lines:
        raise ValueError('zone_set: neither polygons nor lines given')
    if len(polygons) > _lib.ZONES_MAX or len(lines) > _lib.ZONES_MAX:
        raise ValueError(f'zone_set: at most {_lib.ZONES_MAX} polygons and {_lib.ZONES_MAX} lines, got {len(polygons)} and {len(lines)}')
    z = _lib.ZoneSet()
    z.n_polygons, z.n_lines, z.anchor, z.coasting, z.img_h, z.img_w = len(polygons), len(lines), anchor, int(bool(coasting)), h, w
    for p, poly in enumerate(polygons):
        q = _zone_points(f'polygon {p}', poly, 3, _lib.ZONE_MAX_VERTICES).astype(np.int64)
        nxt = np.roll(q, -1, axis=0)
        if int(np.sum(q[:, 0] * nxt[:, 1] - nxt[:, 0] * q[:, 1])) == 0:
            raise ValueError(f'zone_set: polygon {p} has no area at 1/16 pixel: {poly!r}')
        z.n_vertices[p] = len(q)
        for i, (x, y) in enumerate(q.tolist()):
            z.polygon[p][i][0], z.polygon[p][i][1] = x, y
    for l, line in enumerate(lines):
        q = _zone_points(f'line {l}', line, 2, 2)
        if np.array_equal(q[0], q[1]):
            raise ValueError(f'zone_set: line {l} has no length at 1/16 pixel: {line!r}')
        z.line[l][:] = q.reshape(-1).tolist()
    _set_classes('zone_set', z, classes)
    if heat is not None:
        try:
            gh, gw = (int(v) for v in heat)
        except (TypeError, ValueError):
            raise ValueError(f'zone_set: heat is None or (gh, gw), got {heat!r}') from None
        if not (1 <= gh <= _lib.ZONE_MAX_HEAT and 1 <= gw <= _lib.ZONE_MAX_HEAT):
            raise ValueError(f'zone_set: heat (gh, gw) of 1 .. {_lib.ZONE_MAX_HEAT} each expected, got {heat!r}')
        z.heat_h, z.heat_w = gh, gw
    return z


def zones_state_words(max_tracks):
    """int32 words of one stream's zone state (include/mydet.h: mydet_zones_state_words); host arithmetic only."""
    return (_lib.ZONES_STATE_HEADER + _lib.ZONES_SLOT_WORDS * _max_tracks('zones', max_tracks) + 3) // 4 * 4


_ZONES_STATE = _StateFamily('zones', 'zones', zones_state_words, 'max_tracks = {}', 'mydet_zones_reset', _ints, True)


def zones_state(streams, max_tracks, device):
    """A reset zone state: int32 [streams, zones_state_words(max_tracks)] (include/mydet.h has the layout)."""
    return _state_new(_ZONES_STATE, streams, (max_tracks,), device)


def zones_reset_(state, max_tracks):
    """Reset a zone state in place (mydet_zones_reset): nobody inside, every counter and the frame counter 0."""
    return _state_reset(_ZONES_STATE, state, (max_tracks,))


def zones_heat(streams, zone_set, device):
    """A zeroed heat map int32 [streams, gh, gw] for a zone_set with heat=(gh, gw)."""
    if not isinstance(zone_set, _lib.ZoneSet) or zone_set.heat_h < 1:
        raise ValueError('zones_heat: a zone_set(..., heat=(gh, gw)) expected')
    return torch.zeros((int(streams), zone_set.heat_h, zone_set.heat_w), dtype=torch.int32, device=device)


def zones_state_views(state, max_tracks=None):
    """Field views of a zone state int32 [S, words] (include/mydet.h: mydet_zones_frames), nothing copied: a dict of now int32
    [S], zone_counts int32 [S,16,4] (entries, exits, lost, visits), line_counts int32 [S,16,2] (pos, neg), dwell_max int32
    [S,16], dwell_sum int64 [S,16], id int64 [S,MT] (0 = an empty slot), inside, sides, px, py int32 [S,MT], entered int32
    [S,16,MT].  max_tracks: taken from the row length when None.  Works on any device (tests read a host copy)."""
    mt = _row_slots(state, _lib.ZONES_STATE_HEADER, _lib.ZONES_SLOT_WORDS) if max_tracks is None else int(max_tracks)
    _state_check(_ZONES_STATE, state, (mt,), 'zones_state_views', views=True)
    S, Z = state.shape[0], _lib.ZONES_MAX
    out = {'now': state[:, 0], 'zone_counts': state[:, 4:4 + 4 * Z].view(S, Z, 4), 'line_counts': state[:, 4 + 4 * Z:4 + 6 * Z].view(S, Z, 2),
           'dwell_max': state[:, 4 + 6 * Z:4 + 7 * Z], 'dwell_sum': state[:, 4 + 7 * Z:4 + 9 * Z].view(torch.int64)}
    o = _lib.ZONES_STATE_HEADER
    out['id'] = state[:, o:o + 2 * mt].view(torch.int64)
    o += 2 * mt
    for name in ('inside', 'sides', 'px', 'py'):
        out[name] = state[:, o:o + mt]
        o += mt
    out['entered'] = state[:, o:o + Z * mt].view(S, Z, mt)
    return out


def _track_planes(what, track_out, fam, state, *more):
    """(S, F, MT, device) of the dict ops.track_frames returned, its box, id, cls, missed and count planes checked, and with
    them the state of family `fam` (`more`: what its row length takes after MT) that a launch behind the tracker's keeps."""
    box = track_out['box']
    if not isinstance(box, torch.Tensor) or box.dim() != 4 or box.shape[3] != 5:
        raise ValueError(f'{what}: track_out is the dict of ops.track_frames (box [S,F,MT,5], id, cls, missed, count)')
    S, F, mt, _ = box.shape
    dev = box.device
    shapes = {'box': ((S, F, mt, 5), torch.float32), 'id': ((S, F, mt), torch.int64), 'cls': ((S, F, mt), torch.int64),
              'missed': ((S, F, mt), torch.int32), 'count': ((S, F), torch.int32)}
    _check_planes(what, 'track_out', track_out, shapes, dev)
    _state_check(fam, state, (mt,) + more, what)
    if state.shape[0] != S or state.device != dev:
        raise ValueError(f'{what}: a state of {S} streams on {dev} expected, got {state.shape[0]} on {state.device}')
    require_gpu(box, what)
    return S, F, mt, dev


def zones_frames(track_out, state, zone_set, heat=None, out=None):
    """Count the tracks of S streams x F frames in zones and across lines in ONE launch (include/mydet.h: mydet_zones_frames,
    where the rules are).  track_out: the dict ops.track_frames returned (box [S,F,MT,5], id, cls, missed, count are read).
    state: int32 [S, zones_state_words(MT)] from zones_state, updated in place.  zone_set: zone_set(...).  heat: the int32
    [S,gh,gw] buffer of a zone_set with heat= (zones_heat), added to in place; None otherwise.  Returns a dict of int32 device
    tensors, Z polygons and L lines: inside, crossed [S,F,MT], dwell [S,F,MT,Z], occupancy [S,F,Z], zone_counts [S,F,Z,4]
    (entries, exits, lost, visits; cumulative), line_counts [S,F,L,2] (pos, neg; cumulative).  out: such a dict to write into."""
    if not isinstance(zone_set, _lib.ZoneSet):
        raise TypeError(f'zones_frames: zone_set is a _lib.ZoneSet (ops.zone_set), got {type(zone_set).__name__}')
    S, F, mt, dev = _track_planes('zones_frames', track_out, _ZONES_STATE, state)
    if zone_set.heat_h > 0:
        want = (S, zone_set.heat_h, zone_set.heat_w)
        if not isinstance(heat, torch.Tensor) or tuple(heat.shape) != want or heat.dtype != torch.int32 or heat.device != dev or not heat.is_contiguous():
            raise ValueError(f'zones_frames: heat must be a contiguous int32 tensor {want} on {dev} (ops.zones_heat)')
    elif heat is not None:
        raise ValueError('zones_frames: heat given, but the zone_set has no heat grid')
    Z, L = zone_set.n_polygons, zone_set.n_lines
    i32 = torch.int32
    out = out_planes('zones_frames', out, {'inside': ((S, F, mt), i32), 'crossed': ((S, F, mt), i32), 'dwell': ((S, F, mt, Z), i32),
                                           'occupancy': ((S, F, Z), i32), 'zone_counts': ((S, F, Z, 4), i32),
                                           'line_counts': ((S, F, L, 2), i32)}, dev)
    t0 = TIMER.start() if TIMER else None
    code = _lib.lib().mydet_zones_frames(_ptr(track_out['box']), _ptr(track_out['id']), _ptr(track_out['cls']), _ptr(track_out['missed']),
                                         _ptr(track_out['count']), S, F, mt, ctypes.byref(zone_set), _ptr(state), _ptr(heat),
                                         _ptr(out['inside']), _ptr(out['crossed']), _ptr(out['dwell']), _ptr(out['occupancy']),
                                         _ptr(out['zone_counts']), _ptr(out['line_counts']), _stream())
    if t0:
        TIMER.stop('zones_frames', t0, float(S * F))
    _lib.check(code, 'mydet_zones_frames')
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# Camera motion (include/mydet.h: mydet_motion_frames_rgb_u8, where the rules are; csrc/motion.hip)

MOTION_MODELS = {'shift': _lib.MOTION_MODEL_SHIFT, 'similarity': _lib.MOTION_MODEL_SIMILARITY}


def motion_set(reduce=None, search=8, min_texture=1024, min_blocks=None, model='shift', max_zoom=None, max_rotation=None, tolerance=2.0):
    """The settings of the camera-motion estimator (a _lib.MotionSet; include/mydet.h has the rules).  reduce: None (by frame
    size: the smallest of 2, 4, 8 with max(H, W) <= 512 * reduce, else 8) or 2, 4, 8; search: 4 .. 16 reduced pixels;
    min_texture: the least SAD range of a block that counts; min_blocks: None (max(2, ceil(blocks / 8))) or the least number of
    valid blocks of a frame.  model: 'shift' (one integer shift per frame) or 'similarity' (shift, rotation and isotropic zoom,
    mydet_motion_warp_frames_rgb_u8), whose fit takes max_zoom: None (1/8) or the largest |zoom - 1| of a valid frame, up to
    1/4; max_rotation: None (7) or the largest rotation in degrees, up to 14; tolerance: the inlier distance in pixels, up to 16.
    The three are stored as Q16 integers, round(v * 65536).  ValueError for anything out of range, and for a max_zoom, a
    max_rotation or another tolerance with model 'shift'; touches no device."""
    if model not in MOTION_MODELS:
        raise ValueError(f"motion_set: model is 'shift' or 'similarity', got {model!r}")
    def real(name, v, hi):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0 < float(v) <= hi:
            raise ValueError(f'motion_set: 0 < {name} <= {hi} expected, got {v!r}')
        q = int(round(float(v) * 65536))
        if q < 1:
            raise ValueError(f'motion_set: {name} of {v!r} is below 2^-16')
        return q
    fit = (real('tolerance', tolerance, 16.0), 0 if max_zoom is None else real('max_zoom', max_zoom, 0.25),
           0 if max_rotation is None else real('max_rotation', max_rotation, 14.0))
    if model == 'shift' and (max_zoom is not None or max_rotation is not None or fit[0] != 2 << 16):
        raise ValueError("motion_set: max_zoom, max_rotation and tolerance belong to model='similarity'")
    def whole(name, v):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f'motion_set: {name} is an integer, got {v!r}')
        return int(v)
    m = _lib.MotionSet()
    if reduce is not None:
        m.reduce = whole('reduce', reduce)
        if m.reduce not in (2, 4, 8):
            raise ValueError(f'motion_set: reduce is None, 2, 4 or 8, got {reduce!r}')
    m.search = whole('search', search)
    if not _lib.MOTION_MIN_SEARCH <= m.search <= _lib.MOTION_MAX_SEARCH:
        raise ValueError(f'motion_set: search of {_lib.MOTION_MIN_SEARCH} .. {_lib.MOTION_MAX_SEARCH} reduced pixels expected, got {search!r}')
    m.min_texture = whole('min_texture', min_texture)
    if not 0 <= m.min_texture < 1 << 24:
        raise ValueError(f'motion_set: 0 <= min_texture < 2^24 expected, got {min_texture!r}')
    if min_blocks is not None:
        m.min_blocks = whole('min_blocks', min_blocks)
        if not 1 <= m.min_blocks <= _lib.MOTION_MAX_BLOCKS:
            raise ValueError(f'motion_set: min_blocks is None or 1 .. {_lib.MOTION_MAX_BLOCKS}, got {min_blocks!r}')
    if model == 'similarity':                                        # the reserved words stay zero for the shift: today's struct
        m.reserved[0] = _lib.MOTION_MODEL_SIMILARITY
        m.reserved[1], m.reserved[2], m.reserved[3] = fit
    return m


def motion_geometry(frame_hw, set):
    """The geometry the rules give a frame size (H, W) under a motion_set, host arithmetic only: a dict of k, R, hr, wr, wrp (wr
    rounded up to a multiple of 4), nby, nbx, nb, P, min_blocks, state_words.  A ValueError for a frame that is too small for
    2R + 16 reduced pixels per side, too large (32768), or has more than 1024 blocks."""
    if not isinstance(set, _lib.MotionSet):
        raise TypeError(f'motion: set is a _lib.MotionSet (ops.motion_set), got {type(set).__name__}')
    H, W = _frame_hw('motion', frame_hw)
    R = set.search
    k = set.reduce or next((c for c in (2, 4) if max(H, W) <= 512 * c), 8)
    hr, wr = H // k, W // k
    if min(hr, wr) < 2 * R + 16:
        raise ValueError(f'motion: {H}x{W} frames reduced by {k} are {hr}x{wr}, below the 2 * search + 16 = {2 * R + 16} a block and its search window need')
    nby, nbx = (hr - 2 * R) // 16, (wr - 2 * R) // 16
    nb, P, wrp = nby * nbx, min(32, 8 * k), (wr + 3) // 4 * 4
    if nb > _lib.MOTION_MAX_BLOCKS:
        raise ValueError(f'motion: {H}x{W} frames reduced by {k} have {nb} blocks, above {_lib.MOTION_MAX_BLOCKS}; use a larger reduce')
    words = (_lib.MOTION_STATE_HEADER + hr * wrp // 4 + nb * P * P // 4 + 3) // 4 * 4
    return dict(H=H, W=W, k=k, R=R, hr=hr, wr=wr, wrp=wrp, nby=nby, nbx=nbx, nb=nb, P=P,
                min_blocks=set.min_blocks or max(2, (nb + 7) // 8), state_words=words)


# the family's argument is the geometry of a frame size under a motion_set, so that a call works it out once
_MOTION_STATE = _StateFamily('motion', 'motion', lambda geo: geo['state_words'], '{0[H]}x{0[W]} frames', 'mydet_motion_reset',
                             lambda geo: (geo['H'], geo['W'], geo['k'], geo['R']), True)


def motion_state(streams, frame_hw, set, device):
    """A reset estimator state: int32 [streams, words] for frames of frame_hw under `set` (include/mydet.h has the layout)."""
    return _state_new(_MOTION_STATE, streams, (motion_geometry(frame_hw, set),), device)


def motion_reset_(state, frame_hw, set):
    """Reset an estimator state in place (mydet_motion_reset): the next frame of every stream has no previous one."""
    return _state_reset(_MOTION_STATE, state, (motion_geometry(frame_hw, set),))


def motion_state_views(state, frame_hw, set):
    """Field views of an estimator state int32 [S, words], nothing copied: seen int32 [S], reduced uint8 [S,hr,wr] (the last
    frame's reduced luma), patches uint8 [S,nb,P,P].  Works on any device (tests read a host copy)."""
    geo = motion_geometry(frame_hw, set)
    _state_check(_MOTION_STATE, state, (geo,), 'motion_state_views', views=True)
    S, o = state.shape[0], _lib.MOTION_STATE_HEADER
    nred, npat = geo['hr'] * geo['wrp'] // 4, geo['nb'] * geo['P'] ** 2 // 4
    return {'seen': state[:, 0],
            'reduced': state[:, o:o + nred].view(torch.uint8).view(S, geo['hr'], geo['wrp'])[:, :, :geo['wr']],
            'patches': state[:, o + nred:o + nred + npat].view(torch.uint8).view(S, geo['nb'], geo['P'], geo['P'])}


def motion_frames(image, state, set, frames_per_stream=None, layout=None, out=None, inliers=False):
    """The camera motion of S streams x F frames (include/mydet.h: mydet_motion_frames_rgb_u8, where the rules are): per frame
    one integer shift against the frame before it, which for a stream's first frame is the last frame of the previous call
    (kept in `state`).  image: what the ops.draw_* functions take first, read only -- uint8 RGB frames [S*F,H,W,3] with
    packed pixels and any row and frame strides (layout None), or the planes of `layout` ('nv12', 'nv21', 'i420', 'yv12', 'p010',
    'i010') as in yuv420_to_rgb; frame f of stream s is frame s*F + f.  state: motion_state(...), updated in place; its row
    count is S.  frames_per_stream: F, checked against the batch when given.  Returns {'shift': int32 [S,F,4] (dx, dy, valid,
    n_valid), 'blocks': int32 [S,F,nb,6] (cdx, cdy, smin, smax, fdx, fdy)} on the device; out: such a dict to write into.
    With a set of model 'similarity' (mydet_motion_warp_frames_rgb_u8) the dict also holds 'warp': int32 [S,F,8] = (a, b, tx, ty,
    s_q, deg_q, valid, n_inliers), the fitted model in Q16, which track_frames takes as warp=; 'shift' is then the motion of the
    frame centre in whole pixels; inliers=True adds 'inliers': int32 [S,F,nb], the blocks the fit kept (a ValueError with
    model 'shift', before any launch)."""
    what = 'motion_frames'
    if not isinstance(set, _lib.MotionSet):
        raise TypeError(f'{what}: set is a _lib.MotionSet (ops.motion_set), got {type(set).__name__}')
    similarity = set.reserved[0] == _lib.MOTION_MODEL_SIMILARITY
    if inliers and not similarity:
        raise ValueError(f"{what}: inliers are the similarity model's (ops.motion_set(model='similarity'))")
    img, yuv, B = _image(what, image, layout, 'bt601', False, False)
    H, W = (img.shape[1:3] if yuv is None else img[0].shape[1:3])
    geo = motion_geometry((H, W), set)
    _state_check(_MOTION_STATE, state, (geo,), what)
    S = state.shape[0]
    if B % S or (frames_per_stream is not None and int(frames_per_stream) * S != B):
        raise ValueError(f'{what}: {B} frames are not F frames of each of {S} streams')
    F = B // S
    dev = _same_device(what, img, [state])
    shapes = {'shift': ((S, F, 4), torch.int32), 'blocks': ((S, F, geo['nb'], 6), torch.int32)}
    if similarity:
        shapes['warp'] = ((S, F, 8), torch.int32)
        if inliers:
            shapes['inliers'] = ((S, F, geo['nb']), torch.int32)
    out = out_planes(what, out, shapes, dev)
    nbytes = _lib.lib().mydet_motion_workspace_bytes(B, geo['H'], geo['W'], geo['k'], geo['R'])
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    if similarity:
        _launch_on_image(what, img, yuv, 'mydet_motion_warp_frames_rgb_u8', 'mydet_motion_warp_frames_yuv420', S, ctypes.byref(set),
                         _ptr(state), _ptr(ws), nbytes, _ptr(out['shift']), _ptr(out['warp']), _ptr(out['blocks']),
                         _ptr(out['inliers']) if inliers else None)
        return out
    _launch_on_image(what, img, yuv, 'mydet_motion_frames_rgb_u8', 'mydet_motion_frames_yuv420', S, ctypes.byref(set), _ptr(state),
                     _ptr(ws), nbytes, _ptr(out['shift']), _ptr(out['blocks']))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# Key frames (include/mydet.h: mydet_carry_records_rgb_u8, where the rules are; csrc/carry.hip)

def carry_set(every=4, search=8, min_texture=1024, max_diff=24):
    """The settings of the key-frame carry (a _lib.CarrySet; include/mydet.h has the rules).  every: a key frame every n-th
    frame, 1 .. 16; search: the coarse search range, 4 .. 16 cells; min_texture: the least SAD range over a slot's candidates
    that is followed (below it the slot is flat); max_diff: the largest mean absolute difference per cell of a match, 0 .. 255
    (above it the slot is lost).  ValueError for anything out of range; touches no device."""
    def whole(name, v, lo, hi, text):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f'carry_set: {name} is an integer, got {v!r}')
        if not lo <= int(v) <= hi:
            raise ValueError(f'carry_set: {name} of {text} expected, got {v!r}')
        return int(v)
    c = _lib.CarrySet()
    c.every = whole('every', every, 1, _lib.CARRY_MAX_EVERY, f'1 .. {_lib.CARRY_MAX_EVERY} frames')
    c.search = whole('search', search, _lib.MOTION_MIN_SEARCH, _lib.MOTION_MAX_SEARCH, f'{_lib.MOTION_MIN_SEARCH} .. {_lib.MOTION_MAX_SEARCH} cells')
    c.min_texture = whole('min_texture', min_texture, 0, (1 << 24) - 1, '0 .. 2^24 - 1')
    c.max_diff = whole('max_diff', max_diff, 0, 255, '0 .. 255')
    return c


def carry_state_words():
    """int32 words of one stream's carry state: 512 slots of a 16-word header and 1280 template bytes."""
    return _lib.CARRY_SLOTS * _lib.CARRY_SLOT_WORDS


_CARRY_STATE = _StateFamily('carry', 'carry', carry_state_words, '512 slots', 'mydet_carry_reset', lambda: (), True)


def carry_state(streams, device):
    """A reset carry state: int32 zeros [streams, carry_state_words()] -- no slot is carried."""
    return _state_new(_CARRY_STATE, streams, (), device)


def carry_reset_(state):
    """Reset a carry state in place (mydet_carry_reset): the frames before the next key frame carry nothing."""
    return _state_reset(_CARRY_STATE, state, ())


def carry_state_views(state):
    """Field views of a carry state int32 [S, words], nothing copied: status, cell, cx16, cy16 int32 [S,512]; offset, rel int32
    [S,512,2]; box float32 [S,512,4]; angle, score float32 [S,512]; cls int64 [S,512]; coarse uint8 [S,512,16,16]; patch uint8
    [S,512,32,32].  Works on any device (tests read a host copy)."""
    _state_check(_CARRY_STATE, state, (), 'carry_state_views', views=True)
    S = state.shape[0]
    slots = state.view(S, _lib.CARRY_SLOTS, _lib.CARRY_SLOT_WORDS)
    h = _lib.CARRY_SLOT_HEADER
    return {'status': slots[:, :, 0], 'cell': slots[:, :, 1], 'cx16': slots[:, :, 2], 'cy16': slots[:, :, 3],
            'offset': slots[:, :, 4:6], 'rel': slots[:, :, 6:8], 'box': slots[:, :, 8:12].view(torch.float32),
            'angle': slots[:, :, 12].view(torch.float32), 'score': slots[:, :, 13].view(torch.float32),
            'cls': slots[:, :, 14:16].view(torch.int64)[:, :, 0],
            'coarse': slots[:, :, h:h + 64].view(torch.uint8).view(S, _lib.CARRY_SLOTS, 16, 16),
            'patch': slots[:, :, h + 64:h + 320].view(torch.uint8).view(S, _lib.CARRY_SLOTS, 32, 32)}


def carry_first(key_mask, every):
    """The place of a call's frame 0 inside its interval, from the call's key mask (a sequence of F truth values: frame f is a
    key frame): `first` with key_mask[f] == ((first + f) % every == 0).  A ValueError for a mask no `first` gives."""
    mask = [bool(k) for k in key_mask]
    if not mask:
        raise ValueError('carry_records: an empty key mask')
    first = (every - mask.index(True)) % every if True in mask else 1 % every
    if mask != [(first + f) % every == 0 for f in range(len(mask))]:
        raise ValueError(f'carry_records: key mask {mask} is no run of frames with a key frame every {every}')
    return first


def carry_records(source, key_records, key_mask, state, set, frames_per_stream=None, layout=None, shift=None, out=None, records=None):
    """One record per frame out of the records of the key frames (include/mydet.h: mydet_carry_records_rgb_u8, where the rules
    are): a key frame's row is its key record, an in-between row the key boxes carried by their pixels.  source: what the
    ops.draw_* functions take first, read only -- uint8 RGB frames [S*F,H,W,3] with packed pixels and any row and frame
    strides (layout None), or the planes of `layout`; frame f of stream s is frame s*F + f.  key_records: the record dict
    (record_views) or the int32 buffer [S*K, words] of the K key frames of every stream, stream-major, or None when the call
    has no key frame.  key_mask: F truth values, frame f of every stream is a key frame (one every `set.every` frames).
    state: carry_state(...), updated in place; its row count is S.  shift: None, or int32 [S,F,4], the 'shift' of motion_frames
    for the same frames.  Returns the record dict of the [S*F, words] buffer with 'how' int32 [S,F,512], 'offset' and 'sad' int32
    [S,F,512,2] beside it, all on the device; out: a dict with such 'how', 'offset' and 'sad' to write into; records: the int32
    [S*F, words] buffer to write into.  width: 4, or 5 for rotated records, is the key records'; without any it is `records`'."""
    what = 'carry_records'
    if not isinstance(set, _lib.CarrySet):
        raise TypeError(f'{what}: set is a _lib.CarrySet (ops.carry_set), got {type(set).__name__}')
    img, yuv, B = _image(what, source, layout, 'bt601', False, False)
    _state_check(_CARRY_STATE, state, (), what)
    S = state.shape[0]
    if B % S or (frames_per_stream is not None and int(frames_per_stream) * S != B):
        raise ValueError(f'{what}: {B} frames are not F frames of each of {S} streams')
    F = B // S
    mask = list(key_mask)
    if len(mask) != F:
        raise ValueError(f'{what}: a key mask of {F} entries expected, got {len(mask)}')
    first = carry_first(mask, set.every)
    K = sum(bool(k) for k in mask)
    key = key_records
    if isinstance(key, dict):
        key = _record_buffer(what, key)
    if key is None:
        if K:
            raise ValueError(f'{what}: the call has {K} key frames per stream and no key records')
        if records is None:
            raise ValueError(f'{what}: without key records, `records` says the record width')
        words = records.shape[-1]
    else:
        if not isinstance(key, torch.Tensor) or key.dtype != torch.int32 or key.dim() != 2 or key.shape[1] not in (_lib.REC_WORDS, _lib.REC_ROT_WORDS):
            raise ValueError(f'{what}: int32 key records [S*K, {_lib.REC_WORDS} | {_lib.REC_ROT_WORDS}] expected')
        if key.shape[0] != S * K:
            raise ValueError(f'{what}: {S * K} key records ({S} streams x {K} key frames) expected, got {key.shape[0]}')
        if K and (key.stride(1) != 1 or key.stride(0) % 4 or key.stride(0) < key.shape[1]):
            key = key.contiguous()
        words = key.shape[1]
    dev = _same_device(what, img, [state, key, shift, records])
    if shift is not None:
        if not isinstance(shift, torch.Tensor) or shift.dtype != torch.int32 or tuple(shift.shape) != (S, F, 4) or not shift.is_contiguous():
            raise ValueError(f'{what}: shift is a contiguous int32 tensor [{S}, {F}, 4] (motion_frames), got '
                             f'{tuple(shift.shape) if isinstance(shift, torch.Tensor) else type(shift).__name__}')
    if records is None:
        records = torch.empty((B, words), dtype=torch.int32, device=dev)
    if not isinstance(records, torch.Tensor) or records.dtype != torch.int32 or tuple(records.shape) != (B, words) or not records.is_contiguous() \
            or words not in (_lib.REC_WORDS, _lib.REC_ROT_WORDS):
        raise ValueError(f'{what}: records is a contiguous int32 tensor [{B}, {words}]')
    planes = out_planes(what, out, {'how': ((S, F, _lib.CARRY_SLOTS), torch.int32), 'offset': ((S, F, _lib.CARRY_SLOTS, 2), torch.int32),
                                    'sad': ((S, F, _lib.CARRY_SLOTS, 2), torch.int32)}, dev)
    ws = torch.empty((S, _lib.CARRY_SLOTS, 8), dtype=torch.int32, device=dev)
    _launch_on_image(what, img, yuv, 'mydet_carry_records_rgb_u8', 'mydet_carry_records_yuv420', S, ctypes.byref(set), first,
                     _ptr(key) if K else None, key.stride(0) if K else 0, 4 if words == _lib.REC_WORDS else 5, _ptr(state),
                     None if shift is None else _ptr(shift), _ptr(ws), _ptr(records), _ptr(planes['how']), _ptr(planes['offset']),
                     _ptr(planes['sad']))
    res = record_views(records)
    res.update(how=planes['how'], offset=planes['offset'], sad=planes['sad'])
    return res


def bboxes_iou(a, b, xyxy=False):
    require_gpu(a, 'bboxes_iou')
    a, b = a.contiguous().float(), b.contiguous().float()
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    code = _lib.lib().mydet_bboxes_iou_f32(_ptr(a), a.shape[0], _ptr(b), b.shape[0], 1 if xyxy else 0, _ptr(out),
                                           _stream())
    _lib.check(code, 'mydet_bboxes_iou_f32')
    return out


def rotated_iou(a, b):
    """Pairwise IoU [Na, Nb] of rotated boxes, rows (cx, cy, w, h, deg): exact intersection area
    (include/mydet.h: mydet_rotated_iou_f32)."""
    require_gpu(a, 'rotated_iou')
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != 5 or b.shape[1] != 5:
        raise ValueError(f'rotated_iou: [N,5] and [M,5] boxes expected, got {tuple(a.shape)} and {tuple(b.shape)}')
    a, b = a.contiguous().float(), b.to(a.device).contiguous().float()
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    code = _lib.lib().mydet_rotated_iou_f32(_ptr(a), a.shape[0], _ptr(b), b.shape[0], _ptr(out), _stream())
    _lib.check(code, 'mydet_rotated_iou_f32')
    return out


def cxcywh_to_x1y1x2y2(boxes):
    """Rows (cx, cy, w, h[, ...]) -> (x1, y1, x2, y2[, ...]) in a new tensor of the same shape (include/mydet.h:
    mydet_cxcywh_to_x1y1x2y2_f32); any leading dimensions, last dimension >= 4."""
    require_gpu(boxes, 'cxcywh_to_x1y1x2y2')
    if boxes.dtype != torch.float32:
        raise TypeError(f'cxcywh_to_x1y1x2y2: float32 boxes expected, got {boxes.dtype}')
    src = boxes.contiguous()
    out = torch.empty_like(src)
    width = src.shape[-1]
    code = _lib.lib().mydet_cxcywh_to_x1y1x2y2_f32(_ptr(src), _ptr(out), src.numel() // width if width else 0, width, _stream())
    _lib.check(code, 'mydet_cxcywh_to_x1y1x2y2_f32')
    return out


def bboxes_to_original_(bbox, pad_info):
    require_gpu(bbox, 'bboxes_to_original_')
    assert bbox.is_contiguous() and bbox.dtype == torch.float32 and bbox.shape[-1] == 4
    ori_w, ori_h, tl_x, tl_y, imw, imh = [float(v) for v in pad_info]
    code = _lib.lib().mydet_bboxes_to_original_f32(_ptr(bbox), bbox.shape[0], ori_w, ori_h, tl_x, tl_y, imw, imh,
                                                   _stream())
    _lib.check(code, 'mydet_bboxes_to_original_f32')
    return bbox


def resize_bilinear_u8(src_u8, out_hw, dst=None, top=0, left=0):
    """PIL-exact bilinear resize of one uint8 image [H,W,3] on the device (include/mydet.h: mydet_resize_bilinear_u8).
    dst: optional uint8 [Hd,Wd,3] to write into at (top, left) -- e.g. one image of a zero-padded batch buffer."""
    require_gpu(src_u8, 'resize_bilinear_u8')
    assert src_u8.dtype == torch.uint8 and src_u8.dim() == 3 and src_u8.shape[2] == 3 and src_u8.is_contiguous()
    H, W, _ = src_u8.shape
    oh, ow = int(out_hw[0]), int(out_hw[1])
    if dst is None:
        dst = torch.empty((oh, ow, 3), dtype=torch.uint8, device=src_u8.device)
    assert dst.dtype == torch.uint8 and dst.dim() == 3 and dst.shape[2] == 3 and dst.stride(2) == 1 and dst.stride(1) == 3
    assert top + oh <= dst.shape[0] and left + ow <= dst.shape[1]
    (bx, kx, ksx), (by, ky, ksy) = _resample_tables_on(src_u8.device, H, W, oh, ow)
    dptr = ctypes.c_void_p(dst.data_ptr() + top * dst.stride(0) + left * 3)
    code = _lib.lib().mydet_resize_bilinear_u8(_ptr(src_u8), H, W, W * 3, dptr, oh, ow, dst.stride(0), _ptr(bx), _ptr(kx), ksx,
                                               _ptr(by), _ptr(ky), ksy, _stream())
    _lib.check(code, 'mydet_resize_bilinear_u8')
    return dst


_RESAMPLE_CACHE = {}


def _resample_tables_on(device, H, W, oh, ow):
    """Device copies of Pillow's coefficient tables for (H, W) -> (oh, ow), cached per axis and device:
    ((bounds_x, kx, ksx), (bounds_y, ky, ksy)); (None, None, 0) for an axis that keeps its size."""
    from .utils.image_ops import resample_tables
    tabs = []
    for n_in, n_out in ((W, ow), (H, oh)):
        if n_in == n_out:
            tabs.append((None, None, 0))
        else:
            key = (n_in, n_out, str(device))
            hit = _RESAMPLE_CACHE.get(key)
            if hit is None:
                b, k = resample_tables(n_in, n_out)
                hit = (torch.from_numpy(b).to(device), torch.from_numpy(k).to(device), k.shape[1])
                if len(_RESAMPLE_CACHE) > 256:
                    _RESAMPLE_CACHE.clear()
                _RESAMPLE_CACHE[key] = hit
            tabs.append(hit)
    return tabs


def _input_window(what, B, H, W, device, geometry, input_format, out):
    """What frames_to_input and yuv420_to_input (`what`, for the messages) share for B source frames of H x W on `device`:
    (out, (oh, ow), (top, left), taps of the longer filter, the C arguments from `out` to `std3` -- the same run in both
    entry points of include/mydet.h).  out is allocated when None and checked otherwise."""
    norm = _norm_args(input_format)
    target, (top, left), (Hp, Wp), _ = geometry
    oh, ow = (int(target[0]), int(target[1])) if target is not None else (H, W)
    if min(oh, ow) < 1 or top < 0 or left < 0 or top + oh > Hp or left + ow > Wp:
        raise ValueError(f'{what}: a {oh}x{ow} window at ({top}, {left}) does not fit the {Hp}x{Wp} input')
    if out is None:
        out = torch.empty((B, 3, Hp, Wp), dtype=torch.float32, device=device)
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, 3, Hp, Wp) and out.is_contiguous() and out.device == device
    (bx, kx, ksx), (by, ky, ksy) = _resample_tables_on(device, H, W, oh, ow)
    tail = (_ptr(out), Hp, Wp, oh, ow, top, left, _ptr(bx), _ptr(kx), ksx, _ptr(by), _ptr(ky), ksy) + norm
    return out, (oh, ow), (top, left), max(ksx, ksy), tail


def packed_pixels(frames):
    """Whether a kernel can read or write uint8 frames [B,H,W,3] through their strides: the three bytes of a pixel and the
    pixels of a row are packed; any row and frame strides."""
    return frames.stride(3) == 1 and frames.stride(2) == 3 and frames.stride(1) >= 3 * frames.shape[2] and frames.stride(0) >= 0


VIEW_HFLIP, VIEW_VFLIP = _lib.VIEW_HFLIP, _lib.VIEW_VFLIP      # MYDET_VIEW_* of include/mydet.h


def view_flip_bits(flip, what='flip'):
    """The MYDET_VIEW_* bits of a mirrored view: an int 0..3, or '' / 'h' / 'v' / 'hv'.  A ValueError for anything else, raised
    before any device is touched."""
    if isinstance(flip, str):
        if flip not in ('', 'h', 'v', 'hv', 'vh'):
            raise ValueError(f"{what}: a flip is '', 'h', 'v' or 'hv', got {flip!r}")
        return (VIEW_HFLIP if 'h' in flip else 0) | (VIEW_VFLIP if 'v' in flip else 0)
    if isinstance(flip, bool) or not isinstance(flip, int) or not 0 <= flip <= (VIEW_HFLIP | VIEW_VFLIP):
        raise ValueError(f'{what}: flip bits 0..3 (1 = horizontal, 2 = vertical) expected, got {flip!r}')
    return flip


def _flip_dims(flip, first):
    """torch.flip dimensions of the view `flip` for a tensor whose rows are dimension `first`."""
    return [d for d, bit in ((first, VIEW_VFLIP), (first + 1, VIEW_HFLIP)) if flip & bit]


def frames_to_input(frames_u8, geometry, input_format, out=None, flip=0):
    """uint8 frames [B,H,W,3] (or [H,W,3]) of one size on the device -> the float32 network input [B,3,Hp,Wp] in ONE launch
    (include/mydet.h: mydet_frames_to_input_f32): PIL-exact resize, zero padding, /255 and normalisation, the bits
    resize_bilinear_u8 + preprocess_u8 give.  geometry: Detector._geometry's tuple (resize target (h, w) or None,
    (top, left), (Hp, Wp), pad_info).  The frames are read through their strides when pixels are packed (a crop of a
    larger buffer is used in place); a downscale whose filter has more taps than the kernel stages
    (_lib.FRAMES_MAX_TAPS) goes through the two existing kernels instead.  out: optional float32 [B,3,Hp,Wp] view.
    flip: the mirrored view (view_flip_bits: 1 = horizontal, 2 = vertical) -- the bits of this call on torch.flip of the frames,
    read in place by the same launch (mydet_frames_to_input_flip_f32); only the fallback past the tap limit mirrors a copy."""
    flip = view_flip_bits(flip, 'frames_to_input')
    require_gpu(frames_u8, 'frames_to_input')
    if frames_u8.dtype != torch.uint8:
        raise TypeError(f'frames_to_input: uint8 frames expected, got {frames_u8.dtype}')
    if frames_u8.dim() == 3:
        frames_u8 = frames_u8.unsqueeze(0)
    if frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or min(frames_u8.shape) < 1:
        raise ValueError(f'frames_to_input: frames of shape [B,H,W,3] or [H,W,3] expected, got {tuple(frames_u8.shape)}')
    B, H, W, _ = frames_u8.shape
    out, (oh, ow), (top, left), taps, tail = _input_window('frames_to_input', B, H, W, frames_u8.device, geometry, input_format, out)
    if not packed_pixels(frames_u8):
        frames_u8 = frames_u8.contiguous()
    if taps > _lib.FRAMES_MAX_TAPS:
        Hp, Wp = geometry[2]
        buf = torch.zeros((B, Hp, Wp, 3), dtype=torch.uint8, device=frames_u8.device)
        if flip:
            frames_u8 = torch.flip(frames_u8, _flip_dims(flip, 1))
        for n in range(B):
            resize_bilinear_u8(frames_u8[n].contiguous(), (oh, ow), buf[n], top, left)
        return out.copy_(preprocess_u8(buf, (Hp, Wp), input_format))
    head = (_ptr(frames_u8), B, H, W, frames_u8.stride(0), frames_u8.stride(1))
    if flip:
        code = _lib.lib().mydet_frames_to_input_flip_f32(*head, *tail, flip, _stream())
        _lib.check(code, 'mydet_frames_to_input_flip_f32')
        return out
    code = _lib.lib().mydet_frames_to_input_f32(*head, *tail, _stream())
    _lib.check(code, 'mydet_frames_to_input_f32')
    return out


YUV_MATRICES = {'bt601': 0, 'bt709': 1}           # the matrix selector of include/mydet.h, where the coefficient table lives


def yuv_matrix_id(matrix):
    """The C selector of a matrix name; a ValueError for an unknown one (raised before any device is touched)."""
    if matrix not in YUV_MATRICES:
        raise ValueError(f'yuv420: matrix {matrix!r} is not one of {sorted(YUV_MATRICES)}')
    return YUV_MATRICES[matrix]


# layout name -> (selector of include/mydet.h, bytes per sample, planar chroma).  'yv12' is I420 with V stored first: its planes
# are taken in storage order (y, v, u) and exchanged here, so C has no sixth selector.
YUV420_LAYOUTS = {'nv12': (_lib.YUV420_NV12, 1, False), 'nv21': (_lib.YUV420_NV21, 1, False), 'i420': (_lib.YUV420_I420, 1, True),
                  'yv12': (_lib.YUV420_I420, 1, True), 'p010': (_lib.YUV420_P010, 2, False), 'i010': (_lib.YUV420_I010, 2, True)}


def yuv420_layout(layout):
    """(selector, bytes per sample, planar) of a layout name; a ValueError for an unknown one (raised before any device is touched)."""
    if not isinstance(layout, str) or layout not in YUV420_LAYOUTS:
        raise ValueError(f'yuv420: layout {layout!r} is not one of {sorted(YUV420_LAYOUTS)}')
    return YUV420_LAYOUTS[layout]


def yuv420_sample_dtypes(bps):
    """The torch dtypes a plane of `bps` bytes per sample may have: uint8; int16 (the same bits) and, where this torch has it, uint16."""
    if bps == 1:
        return (torch.uint8,)
    return (torch.int16,) + ((torch.uint16,) if hasattr(torch, 'uint16') else ())


def yuv420_plane_shapes(layout, B, H, W):
    """The shapes of the planes of B frames of H x W: Y, then one interleaved chroma plane or two planar ones."""
    _, _, planar = yuv420_layout(layout)
    ch, cw = (H + 1) // 2, (W + 1) // 2
    return [(B, H, W)] + ([(B, ch, cw)] * 2 if planar else [(B, ch, cw, 2)])


def yuv420_samples(t, layout, what):
    """One plane of `layout` as the tensor the kernels read: a TypeError, worded with `what` (the caller), for anything but a
    tensor of the layout's dtype; uint16 words come back as an int16 view of the same bits.  Touches no device."""
    dtypes = yuv420_sample_dtypes(yuv420_layout(layout)[1])
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes:
        raise TypeError(f"{what}: {layout!r} planes are tensors of dtype {' or '.join(str(d) for d in dtypes)}, got "
                        f'{t.dtype if isinstance(t, torch.Tensor) else type(t).__name__}')
    return t if t.dtype in (torch.uint8, torch.int16) else t.view(torch.int16)


def yuv420_check_planes(planes, layout, what):
    """The rules every list of planes of `layout` meets, on any device and touching none: (the planes [y [B,H,W], chroma or
    u(, v)] in the order given, 2-d input?).  Each plane by yuv420_samples, the layout's number of planes, 2-d planes mean
    one frame, chroma of yuv420_plane_shapes.  Errors in that order, worded with `what` (the caller)."""
    planar = yuv420_layout(layout)[2]
    planes = [yuv420_samples(t, layout, what) for t in planes]
    names = '(y, u, v)' if planar else '(y, uv)'
    if len(planes) != (3 if planar else 2):
        raise ValueError(f'{what}: {layout!r} takes the planes {names}, got {len(planes)}')
    single = planes[0].dim() == 2
    if single:
        planes = [t.unsqueeze(0) if t.dim() == (2 if planar or i == 0 else 3) else t for i, t in enumerate(planes)]
    y = planes[0]
    if y.dim() != 3 or min(y.shape) < 1:
        raise ValueError(f'{what}: a Y plane of shape [B,H,W] or [H,W] expected, got {tuple(y.shape)}')
    want = yuv420_plane_shapes(layout, *y.shape)
    for t, shape in zip(planes[1:], want[1:]):
        if tuple(t.shape) != shape:
            raise ValueError(f'{what}: {layout!r} chroma planes of shape {shape} expected for Y {tuple(y.shape)}, got {tuple(t.shape)}')
    return planes, single


def _yuv420_planes(planes, layout, what, in_place=False):
    """What every kernel on 4:2:0 frames shares: the checked planes (yuv420_check_planes) in the order of
    mydet_yuv420_src.plane and whether the input was 2-d; on the device, used in place through their frame and row strides
    when samples (and pairs) are packed -- planes that are not are copied, or refused (ValueError) when the kernel writes them
    (in_place).  Type, dtype, shape and in-place errors are raised before any device is touched."""
    if not isinstance(planes, (tuple, list)):
        raise TypeError(f'{what}: a tuple of planes expected, got {type(planes).__name__}')
    planes, single = yuv420_check_planes(planes, layout, what)
    for i, t in enumerate(planes):
        inner = t.dim() == 4                                             # pairs: the last two dimensions are packed
        packed = t.stride(-1) == 1 and (not inner or t.stride(2) == 2) and t.stride(1) >= t.shape[2] * (2 if inner else 1) and t.stride(0) >= 0
        if in_place and not packed:
            raise ValueError(f'{what}: planes are drawn in place and need packed samples (strides {tuple(t.stride())} of {tuple(t.shape)})')
        require_gpu(t, what)
        if t.device != planes[0].device:
            raise ValueError(f'{what}: y is on {planes[0].device}, another plane on {t.device}')
        if not packed:
            planes[i] = t.contiguous()
    if layout == 'yv12':
        planes[1], planes[2] = planes[2], planes[1]
    return planes, single


def _yuv420_src(planes, layout, matrix, full_range):
    """mydet_yuv420_src of checked planes (_yuv420_planes)."""
    sel, bps, _ = yuv420_layout(layout)
    src = _lib.Yuv420Src()
    for i, t in enumerate(planes):
        src.plane[i], src.img_bytes[i], src.row_bytes[i] = _ptr(t), t.stride(0) * bps, t.stride(1) * bps
    src.layout, src.matrix, src.full_range = sel, matrix, int(bool(full_range))
    return src


def yuv420_to_rgb(planes, layout, matrix='bt601', full_range=False, out=None):
    """4:2:0 frames on the device -> packed uint8 RGB [B,H,W,3] ([H,W,3] for 2-d planes) (include/mydet.h:
    mydet_yuv420_to_rgb_u8, where the layouts, the 10-bit rule and the formula are).  layout: 'nv12', 'nv21', 'p010' with
    planes (y [B,H,W], uv [B,ceil(H/2),ceil(W/2),2]); 'i420', 'i010' with (y, u, v), 'yv12' with (y, v, u), chroma planes
    [B,ceil(H/2),ceil(W/2)].  uint8 for the 8-bit layouts, int16 or uint16 words for 'p010' / 'i010'.  Samples (and pairs)
    packed, any row and frame strides, read in place.  matrix: 'bt601' or 'bt709'; full_range: Y in 0..255 instead of 16..235.
    out: optional uint8 [B,H,W,3] view with packed pixels."""
    yuv420_layout(layout)
    m = yuv_matrix_id(matrix)
    planes, single = _yuv420_planes(planes, layout, 'yuv420_to_rgb')
    B, H, W = planes[0].shape
    if out is None:
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=planes[0].device)
    dst = out.unsqueeze(0) if out.dim() == 3 else out
    assert dst.dtype == torch.uint8 and tuple(dst.shape) == (B, H, W, 3) and dst.device == planes[0].device
    assert packed_pixels(dst)
    src = _yuv420_src(planes, layout, m, full_range)
    code = _lib.lib().mydet_yuv420_to_rgb_u8(ctypes.byref(src), B, H, W, _ptr(dst), dst.stride(0), dst.stride(1), _stream())
    _lib.check(code, 'mydet_yuv420_to_rgb_u8')
    return dst[0] if single else dst


def yuv420_to_input(planes, layout, geometry, input_format, matrix='bt601', full_range=False, out=None, flip=0):
    """4:2:0 frames of one size on the device -> the float32 network input [B,3,Hp,Wp] in ONE launch (include/mydet.h:
    mydet_yuv420_to_input_f32): the bits of frames_to_input(yuv420_to_rgb(planes, layout, matrix, full_range), geometry,
    input_format) without the RGB frames.  planes, layout, matrix, full_range as in yuv420_to_rgb; geometry, input_format,
    out and the tap limit as in frames_to_input -- past the limit the frames are converted and go through frames_to_input's
    own fallback.  flip: the mirrored view (view_flip_bits), by mydet_yuv420_to_input_flip_f32: the mirrored RGB frames of
    yuv420_to_rgb, chroma fetched at the pixel's own position in the planes."""
    flip = view_flip_bits(flip, 'yuv420_to_input')
    yuv420_layout(layout)
    m = yuv_matrix_id(matrix)
    checked, _ = _yuv420_planes(planes, layout, 'yuv420_to_input')
    B, H, W = checked[0].shape
    out, _, _, taps, tail = _input_window('yuv420_to_input', B, H, W, checked[0].device, geometry, input_format, out)
    if taps > _lib.FRAMES_MAX_TAPS:
        return frames_to_input(yuv420_to_rgb(planes, layout, matrix, full_range), geometry, input_format, out, flip)
    src = _yuv420_src(checked, layout, m, full_range)
    if flip:
        code = _lib.lib().mydet_yuv420_to_input_flip_f32(ctypes.byref(src), B, H, W, *tail, flip, _stream())
        _lib.check(code, 'mydet_yuv420_to_input_flip_f32')
        return out
    code = _lib.lib().mydet_yuv420_to_input_f32(ctypes.byref(src), B, H, W, *tail, _stream())
    _lib.check(code, 'mydet_yuv420_to_input_f32')
    return out


def nv12_to_rgb(y, uv, matrix='bt601', full_range=False, out=None):
    """NV12 frames on the device -> packed uint8 RGB [B,H,W,3] ([H,W,3] for a 2-d y) (include/mydet.h: mydet_nv12_to_rgb_u8,
    where the formula and the coefficient table are).  y: uint8 [B,H,W] or [H,W], element stride 1 along W; uv: uint8
    [B,ceil(H/2),ceil(W/2),2], last two dimensions packed; any row and frame strides, read in place.  matrix: 'bt601' or
    'bt709'; full_range: Y in 0..255 instead of 16..235.  out: optional uint8 [B,H,W,3] view with packed pixels."""
    return yuv420_to_rgb((y, uv), 'nv12', matrix, full_range, out)


def nv12_to_input(y, uv, geometry, input_format, matrix='bt601', full_range=False, out=None):
    """NV12 frames of one size on the device -> the float32 network input [B,3,Hp,Wp] in ONE launch (include/mydet.h:
    mydet_nv12_to_input_f32): the bits of frames_to_input(nv12_to_rgb(y, uv, matrix, full_range), geometry, input_format)
    without the RGB frames.  y, uv, matrix, full_range as in nv12_to_rgb; geometry, input_format, out and the tap limit as
    in frames_to_input -- past the limit the frames are converted and go through frames_to_input's own fallback."""
    return yuv420_to_input((y, uv), 'nv12', geometry, input_format, matrix, full_range, out)


def records_to_original_(rec, pad_infos):
    """bboxes_to_original_ for a whole batch of records in place: pad_infos = one (ori w, ori h, tl x, tl y, imw, imh)
    per image (a row of ones-and-zeros (1, 1, 0, 0, 1, 1) leaves an image's boxes unchanged bit for bit)."""
    bbox = rec['bbox']
    require_gpu(bbox, 'records_to_original_')
    B, K = bbox.shape[0], bbox.shape[1]
    pad = torch.tensor([[float(v) for v in p] if p is not None else [1.0, 1.0, 0.0, 0.0, 1.0, 1.0] for p in pad_infos],
                       dtype=torch.float32).to(bbox.device, non_blocking=True)
    assert pad.shape == (B, 6) and bbox.stride(1) == 4 and bbox.stride(2) == 1
    code = _lib.lib().mydet_bboxes_to_original_batched_f32(_ptr(bbox), bbox.stride(0), _ptr(rec['count']), rec['count'].stride(0),
                                                           B, K, _ptr(pad), _stream())
    _lib.check(code, 'mydet_bboxes_to_original_batched_f32')
    return rec


def detections_to_json(bbox, score, cls, count=None, cat_table=None):
    """The numbers of ImageObjects.to_json for B x K detection slots in one launch: returns (rows float64 [B,K,5] =
    x1, y1, w, h, score in the reference's double arithmetic, category int64 [B,K]).  bbox [B,K,4] (any image
    stride), score [B,K], cls [B,K] int64, count [B] int32 or None, cat_table int64 [n] or None."""
    require_gpu(bbox, 'detections_to_json')
    B, K = bbox.shape[0], bbox.shape[1]
    out = torch.empty((B, K, 5), dtype=torch.float64, device=bbox.device)
    cat = torch.empty((B, K), dtype=torch.int64, device=bbox.device)
    if K == 0:
        return out, cat
    assert bbox.stride(1) == 4 and bbox.stride(2) == 1 and score.stride(1) == 1 and cls.stride(1) == 1
    code = _lib.lib().mydet_detections_to_json_f64(_ptr(bbox), bbox.stride(0), _ptr(score), score.stride(0), _ptr(cls),
                                                   cls.stride(0), _ptr(count), count.stride(0) if count is not None else 0,
                                                   B, K, _ptr(cat_table), cat_table.numel() if cat_table is not None else 0,
                                                   _ptr(out), _ptr(cat), _stream())
    _lib.check(code, 'mydet_detections_to_json_f64')
    return out, cat


IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
_MEAN_F32 = np.asarray(IMAGENET_MEAN, dtype=np.float32)          # module-level: the kernels' launch reads them through pointers
_STD_F32 = np.asarray(IMAGENET_STD, dtype=np.float32)


def _norm_args(input_format):
    """The (norm, mean3, std3) arguments of the input kernels for an input format."""
    if input_format not in ('RGB_1', 'RGB_1_norm'):
        raise NotImplementedError()
    return 1 if input_format == 'RGB_1_norm' else 0, ctypes.c_void_p(_MEAN_F32.ctypes.data), ctypes.c_void_p(_STD_F32.ctypes.data)


def preprocess_u8(img_u8, out_hw, input_format):
    """uint8 [B,H,W,3] (or [H,W,3]) device tensor -> float32 [B,3,Hp,Wp]: zero-pad right/bottom, /255, and for
    'RGB_1_norm' the ImageNet normalisation -- the tensor the reference builds on the host with tvf.pad +
    tvf.to_tensor + format_tensor_img (api/detection.py:158-163)."""
    require_gpu(img_u8, 'preprocess_u8')
    if img_u8.dim() == 3:
        img_u8 = img_u8.unsqueeze(0)
    assert img_u8.dtype == torch.uint8 and img_u8.shape[-1] == 3
    img_u8 = img_u8.contiguous()
    B, H, W, _ = img_u8.shape
    Hp, Wp = out_hw
    out = torch.empty((B, 3, Hp, Wp), dtype=torch.float32, device=img_u8.device)
    code = _lib.lib().mydet_preprocess_u8_f32(_ptr(img_u8), B, H, W, _ptr(out), Hp, Wp, *_norm_args(input_format), _stream())
    _lib.check(code, 'mydet_preprocess_u8_f32')
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# Overlay renderer (include/mydet.h: mydet_draw_boxes_rgb_u8 / mydet_draw_boxes_yuv420_u8, where the raster rules are).
# draw_palette, rgb_to_yuv and draw_label_text are host functions and ARE the documented rules for colour and text.

DRAW_LABELS = {'class': _lib.DRAW_LABEL_CLASS, 'score': _lib.DRAW_LABEL_SCORE, 'id': _lib.DRAW_LABEL_ID}
DRAW_COLOR_MODES = {'class': _lib.DRAW_COLOR_CLASS, 'id': _lib.DRAW_COLOR_ID, 'fixed': _lib.DRAW_COLOR_FIXED}
# RGB -> Y'CbCr rows with 8 fraction bits, (matrix id, full range) -> (Y row, U row, V row, luma offset): the table of include/mydet.h
DRAW_YUV_ROWS = {(0, 0): ((66, 129, 25), (-38, -74, 112), (112, -94, -18), 16),
                 (0, 1): ((77, 150, 29), (-43, -85, 128), (128, -107, -21), 0),
                 (1, 0): ((47, 157, 16), (-26, -86, 112), (112, -102, -10), 16),
                 (1, 1): ((54, 183, 18), (-29, -99, 128), (128, -116, -12), 0)}
DRAW_PALETTE_HUES, DRAW_PALETTE_STEP = 1530, 946


def draw_palette(n=256):
    """The colour table of the renderer, uint8 numpy [n, 3], by integer arithmetic alone: entry i is the fully saturated,
    full-value colour of hue h = (i * 946) mod 1530 on a wheel of 6 * 255 steps (946 / 1530 is the golden-ratio step), i.e.
    with sector = h // 255 and f = h % 255 the channels (255, f, 0), (255 - f, 255, 0), (0, 255, f), (0, 255 - f, 255),
    (f, 0, 255), (255, 0, 255 - f) for sectors 0..5.  Deterministic; entries are pairwise distinct for n <= 765."""
    n = int(n)
    if n < 1:
        raise ValueError(f'draw_palette: n >= 1 expected, got {n}')
    h = (np.arange(n, dtype=np.int64) * DRAW_PALETTE_STEP) % DRAW_PALETTE_HUES
    sector, f = h // 255, h % 255
    up, down, hi, lo = f, 255 - f, np.full(n, 255), np.zeros(n, dtype=np.int64)
    r = np.choose(sector, [hi, down, lo, lo, up, hi])
    g = np.choose(sector, [up, hi, hi, down, lo, lo])
    b = np.choose(sector, [lo, lo, up, hi, hi, down])
    return np.stack([r, g, b], axis=1).astype(np.uint8)


def rgb_to_yuv(rgb, matrix='bt601', full_range=False):
    """uint8 RGB [..., 3] (numpy) -> uint8 (Y, U, V) [..., 3] by the renderer's fixed-point rows (include/mydet.h):
    Y = ((yr R + yg G + yb B + 128) >> 8) + (0 | 16), U = ((...) >> 8) + 128, V likewise, each clamped to 0..255."""
    yr, ur, vr, yoff = DRAW_YUV_ROWS[(yuv_matrix_id(matrix), int(bool(full_range)))]
    c = np.asarray(rgb).astype(np.int64)
    if c.shape[-1] != 3:
        raise ValueError(f'rgb_to_yuv: [..., 3] expected, got {c.shape}')
    out = [((c * np.asarray(row, dtype=np.int64)).sum(-1) + 128 >> 8) + off for row, off in ((yr, yoff), (ur, 128), (vr, 128))]
    return np.clip(np.stack(out, axis=-1), 0, 255).astype(np.uint8)


def draw_label_flags(labels):
    """The C label flags of an iterable of 'class' / 'score' / 'id' (or of the flags themselves); a ValueError otherwise."""
    if isinstance(labels, (int, np.integer)) and not isinstance(labels, bool):
        if not 0 <= int(labels) <= 7:
            raise ValueError(f'draw: label flags in 0..7 expected, got {labels}')
        return int(labels)
    if labels is None:
        return 0
    if isinstance(labels, str):
        labels = (labels,)
    flags = 0
    for name in labels:
        if not isinstance(name, str) or name not in DRAW_LABELS:
            raise ValueError(f'draw: label {name!r} is not one of {sorted(DRAW_LABELS)}')
        flags |= DRAW_LABELS[name]
    return flags


def draw_label_text(cls=None, score=None, id=None, names=None, flags=('class', 'score', 'id')):
    """The text the renderer writes for one row (the rule of include/mydet.h as host code).  Parts in the order class, score,
    id, one space between two parts; a part that is not in `flags`, whose value is None or that is empty is left out.  class: names[cls]
    cut to 16 characters when `names` is given and 0 <= cls < len(names), else the decimal class index cut to 16 characters;
    score: d.dd of min(100, floor(score * 100 + 0.5)) in float32, 0.00 for NaN or a score <= 0; id: '#' and id mod 10^10."""
    flags = draw_label_flags(flags)
    parts = []
    if flags & _lib.DRAW_LABEL_CLASS and cls is not None:
        c = int(cls)
        parts.append((str(names[c]) if names is not None and 0 <= c < len(names) else str(c))[:_lib.DRAW_NAME_BYTES])
    if flags & _lib.DRAW_LABEL_SCORE and score is not None:
        s, v = np.float32(score), 0
        if s > 0:                                                    # NaN compares false
            f = np.float32(np.float32(s * np.float32(100.0)) + np.float32(0.5))
            v = 100 if f >= 100 else int(np.floor(f))
        parts.append(f'{v // 100}.{v // 10 % 10}{v % 10}')
    if flags & _lib.DRAW_LABEL_ID and id is not None:
        parts.append(f'#{int(id) % 10 ** 10}')
    return ' '.join(p for p in parts if p)


_ATLAS_HOST = {}
_ATLAS_DEVICE = {}


def _glyph_atlas_host(height):
    """uint8 numpy [96, height, cw] of 0 / 1: ASCII 32..127, one glyph per fixed cell, rendered with Pillow's default font without
    anti-aliasing and binarised at 128.  Sized (FreeType) when this Pillow has ImageFont.load_default(size=): the largest size at which the ink of
    every glyph fits the rows; otherwise the built-in bitmap font, repeated by the whole factor that fits."""
    if height in _ATLAS_HOST:
        return _ATLAS_HOST[height]
    from PIL import Image, ImageDraw, ImageFont
    chars = [chr(c) for c in range(32, 127)]                         # 127 (DEL) has no glyph: an empty cell
    font, scale, boxes = None, 1, None
    try:
        for size in range(2 * height, 3, -1):                        # the largest size whose ink (all glyphs) fits the rows
            f = ImageFont.load_default(size=size)
            bs = [f.getbbox(c, mode='1') for c in chars]
            if max(b[3] for b in bs) - min(b[1] for b in bs) <= height:
                font, boxes = f, bs
                break
    except (TypeError, AttributeError, OSError):
        font = None
    if font is None:
        font = ImageFont.load_default()
        boxes = [font.getbbox(c) for c in chars]
        scale = max(1, height // max(1, max(b[3] for b in boxes) - min(b[1] for b in boxes)))
    x0, y0 = min(b[0] for b in boxes), min(b[1] for b in boxes)
    cell_w = max(1, max(b[2] for b in boxes) - x0)
    cell_h = max(1, -(-height // scale))
    top = max(0, (cell_h - (max(b[3] for b in boxes) - y0)) // 2)
    atlas = np.zeros((96, height, cell_w * scale), dtype=np.uint8)
    for k, c in enumerate(chars):
        img = Image.new('L', (cell_w, cell_h), 0)
        pen = ImageDraw.Draw(img)
        pen.fontmode = '1'                                           # hinted, not anti-aliased: thin strokes survive at small sizes
        pen.text((-x0, top - y0), c, fill=255, font=font)
        g = (np.asarray(img) >= 128).astype(np.uint8)
        g = np.repeat(np.repeat(g, scale, axis=0), scale, axis=1)[:height]
        atlas[k, :g.shape[0]] = g
    _ATLAS_HOST[height] = atlas
    return atlas


def glyph_atlas(height, device=None):
    """The renderer's monospace glyph atlas for label cells of `height` rows (8..64): uint8 [96, height, cw] of 0 / 1 for
    ASCII 32..127, built at run time on the host from Pillow's default font (no font file ships with the package) and cached
    per (device, height).  device=None: the host tensor."""
    height = int(height)
    if not 8 <= height <= 64:
        raise ValueError(f'glyph_atlas: a cell height in 8..64 expected, got {height}')
    host = _glyph_atlas_host(height)
    if host.shape[2] > 64:
        raise ValueError(f'glyph_atlas: cells of height {height} are {host.shape[2]} wide; the renderer takes at most 64')
    if device is None:
        return torch.from_numpy(host)
    key = (str(torch.device(device)), height)
    if key not in _ATLAS_DEVICE:
        _ATLAS_DEVICE[key] = torch.from_numpy(host).to(device)
    return _ATLAS_DEVICE[key]


class DrawStyle:
    """What ops.draw_style returns: the checked settings on the host; the device tables (palette, atlas, names) are made the
    first time a device draws with it."""

    def __init__(self, thickness, fill_alpha, color_mode, color, labels, label_height, names, n_palette):
        self.thickness, self.fill_alpha, self.color_mode, self.color = thickness, fill_alpha, color_mode, color
        self.label_flags, self.label_height, self.names, self.n_palette = labels, label_height, names, n_palette
        self._tables = {}

    def __repr__(self):
        return (f'DrawStyle(thickness={self.thickness}, fill_alpha={self.fill_alpha}, color_mode={self.color_mode}, color={self.color}, '
                f'label_flags={self.label_flags}, label_height={self.label_height}, names={None if self.names is None else len(self.names)})')

    def struct(self, device):
        """(mydet_draw_style for `device`, the tensors it points to)."""
        key = str(torch.device(device))
        if key not in self._tables:
            palette = torch.from_numpy(draw_palette(self.n_palette)).to(device)
            atlas = glyph_atlas(self.label_height, device) if self.label_flags else None
            names = None
            if self.names is not None and len(self.names):
                table = np.zeros((len(self.names), _lib.DRAW_NAME_BYTES), dtype=np.uint8)
                for k, name in enumerate(self.names):
                    raw = name.encode('ascii', 'replace')[:_lib.DRAW_NAME_BYTES]
                    table[k, :len(raw)] = np.frombuffer(raw, dtype=np.uint8)
                names = torch.from_numpy(table).to(device)
            self._tables[key] = (palette, atlas, names)
        palette, atlas, names = self._tables[key]
        s = _lib.DrawStyle()
        s.thickness, s.fill_alpha, s.color_mode, s.label_flags = self.thickness, self.fill_alpha, self.color_mode, self.label_flags
        s.color[:] = list(self.color) + [0]
        s.n_palette, s.palette = palette.shape[0], _ptr(palette)
        if atlas is not None:
            s.atlas, s.ch, s.cw = _ptr(atlas), atlas.shape[1], atlas.shape[2]
        if names is not None:
            s.names, s.n_names = _ptr(names), names.shape[0]
        return s, (palette, atlas, names)


def draw_style(thickness=2, fill_alpha=0, color_by='class', color=None, labels=(), label_height=16, class_names=None, n_palette=256):
    """The settings of a draw call, checked here and touching no device (a DrawStyle).  thickness: the outline's, 1..64 pixels;
    fill_alpha: 0 (no fill) .. 255; color_by: 'class' or 'id' (palette[key mod n_palette], ops.draw_palette) or 'fixed';
    color: (r, g, b) -- given, it implies 'fixed'; labels: any of 'class', 'score', 'id'; label_height: rows of a label cell, 8..64
    (ops.glyph_atlas); class_names: a list of ASCII names (16 characters are shown), None = the class index is shown."""
    if isinstance(thickness, bool) or not isinstance(thickness, (int, np.integer)) or not 1 <= thickness <= _lib.DRAW_MAX_THICKNESS:
        raise ValueError(f'draw_style: an integer thickness in 1..{_lib.DRAW_MAX_THICKNESS} expected, got {thickness!r}')
    if isinstance(fill_alpha, bool) or not isinstance(fill_alpha, (int, np.integer)) or not 0 <= fill_alpha <= 255:
        raise ValueError(f'draw_style: an integer fill_alpha in 0..255 expected, got {fill_alpha!r}')
    if color is not None:
        color_by = 'fixed'
        c = tuple(color) if isinstance(color, (tuple, list, np.ndarray)) else None
        if c is None or len(c) != 3 or any(isinstance(v, (bool, float)) or not 0 <= int(v) <= 255 for v in c):
            raise ValueError(f'draw_style: color = (r, g, b) of integers in 0..255 expected, got {color!r}')
        color = tuple(int(v) for v in c)
    if not isinstance(color_by, str) or color_by not in DRAW_COLOR_MODES:
        raise ValueError(f'draw_style: color_by {color_by!r} is not one of {sorted(DRAW_COLOR_MODES)}')
    if color_by == 'fixed' and color is None:
        raise ValueError("draw_style: color_by 'fixed' needs color = (r, g, b)")
    flags = draw_label_flags(labels)
    label_height = int(label_height)
    if not 8 <= label_height <= 64:
        raise ValueError(f'draw_style: a label_height in 8..64 expected, got {label_height}')
    if class_names is not None:
        class_names = list(class_names)
        if not all(isinstance(n, str) for n in class_names):
            raise TypeError('draw_style: class_names is a list of str')
    n_palette = int(n_palette)
    if n_palette < 1:
        raise ValueError(f'draw_style: n_palette >= 1 expected, got {n_palette}')
    return DrawStyle(int(thickness), int(fill_alpha), DRAW_COLOR_MODES[color_by], color or (0, 0, 0), flags, label_height, class_names, n_palette)


def _draw_check_style(style, what):
    if not isinstance(style, DrawStyle):
        raise TypeError(f'{what}: style is an ops.DrawStyle (ops.draw_style), got {type(style).__name__}')


def _box_rows(what, B, boxes, counts, scores, classes, ids):
    """The checked dense row tensors of a draw or crop call (no device touched): boxes [B,K,4|5] float32 and the optional planes."""
    if not isinstance(boxes, torch.Tensor) or boxes.dtype != torch.float32:
        raise TypeError(f'{what}: boxes is a float32 tensor, got {boxes.dtype if isinstance(boxes, torch.Tensor) else type(boxes).__name__}')
    if boxes.dim() == 2:
        boxes = boxes.unsqueeze(0)
    if boxes.dim() != 3 or boxes.shape[2] not in (4, 5) or boxes.shape[0] != B:
        raise ValueError(f'{what}: boxes of shape [{B},K,4|5] (or [K,4|5] for one frame) expected, got {tuple(boxes.shape)}')
    K = boxes.shape[1]
    planes = {}
    for name, t, dt in (('scores', scores, torch.float32), ('classes', classes, torch.int64), ('ids', ids, torch.int64)):
        if t is None:
            planes[name] = None
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise TypeError(f'{what}: {name} is a {dt} tensor, got {t.dtype if isinstance(t, torch.Tensor) else type(t).__name__}')
        t = t.unsqueeze(0) if t.dim() == 1 else t
        if tuple(t.shape) != (B, K):
            raise ValueError(f'{what}: {name} of shape [{B},{K}] expected, got {tuple(t.shape)}')
        planes[name] = t
    if counts is not None:
        if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32:
            raise TypeError(f'{what}: counts is an int32 tensor, got {counts.dtype if isinstance(counts, torch.Tensor) else type(counts).__name__}')
        counts = counts.reshape(-1)
        if counts.shape[0] != B:
            raise ValueError(f'{what}: counts of shape [{B}] expected, got {tuple(counts.shape)}')
    return boxes, counts, planes


def _image(what, image, layout, matrix, full_range, in_place):
    """The image side of a draw or crop call: (what the kernel is given -- the uint8 frames [B,H,W,3] (layout None) or the
    checked planes of `layout` (_yuv420_planes) --, None or (layout, matrix id, full_range), B).  Frames and planes are used
    through their strides when pixels or samples are packed; those that are not are copied, or, when the kernel writes them
    (in_place), refused with a ValueError, as the 10-bit layouts then are."""
    if layout is not None:
        if yuv420_layout(layout)[1] != 1 and in_place:
            raise ValueError(f'{what}: layout {layout!r} is not drawn into; the 8-bit layouts nv12, nv21, i420 and yv12 are')
        m = yuv_matrix_id(matrix)
        planes, _ = _yuv420_planes(image, layout, what, in_place)
        return planes, (layout, m, full_range), planes[0].shape[0]
    if not isinstance(image, torch.Tensor) or image.dtype != torch.uint8:
        raise TypeError(f'{what}: uint8 frames expected, got {image.dtype if isinstance(image, torch.Tensor) else type(image).__name__}')
    fr = image.unsqueeze(0) if image.dim() == 3 else image
    if fr.dim() != 4 or fr.shape[3] != 3 or min(fr.shape) < 1:
        raise ValueError(f'{what}: frames of shape [B,H,W,3] or [H,W,3] expected, got {tuple(image.shape)}')
    if not packed_pixels(fr):
        if in_place:
            raise ValueError(f'{what}: frames are drawn in place and need packed pixels (strides {tuple(fr.stride())} of {tuple(fr.shape)})')
        fr = fr.contiguous()
    return fr, None, fr.shape[0]


def _same_device(what, image, tensors):
    """The device of the frames or planes of _image, which every tensor of `tensors` (None entries aside) shares."""
    planes = [image] if isinstance(image, torch.Tensor) else list(image)
    dev = planes[0].device
    for t in planes + [t for t in tensors if t is not None]:
        require_gpu(t, what)
        if t.device != dev:
            raise ValueError(f'{what}: the target is on {dev}, another tensor on {t.device}')
    return dev


def _list_of_records(what, records, labels, ids):
    """The _lib.DrawList of a checked records buffer (_record_buffer), read in place through its strides: the boxes, the
    angles of rotated records and the counts; with `labels` the score and class planes as well.  ids: None, or a contiguous
    int64 [B,512] that the caller keeps alive."""
    base, fs = records.data_ptr(), records.stride(0)
    lst = _lib.DrawList()
    lst.box, lst.box_frame_stride, lst.box_row_stride = base + 4 * _lib.REC_BBOX, fs, 4
    if records.shape[1] == _lib.REC_ROT_WORDS:
        lst.angle, lst.angle_frame_stride, lst.angle_row_stride = base + 4 * _lib.REC_ANGLE, fs, 1
    if labels:
        if fs % 2:
            raise ValueError(f'{what}: a record stride of an even number of words expected, got {fs}')
        lst.score, lst.score_frame_stride, lst.score_row_stride = base + 4 * _lib.REC_SCORE, fs, 1
        lst.cls, lst.cls_frame_stride, lst.cls_row_stride = base + 4 * _lib.REC_CLASS, fs // 2, 1      # int64 elements: fs is even
    if ids is not None:
        lst.id, lst.id_frame_stride, lst.id_row_stride = _ptr(ids), _lib.REC_TOPK, 1
    lst.count, lst.count_stride = base + 4 * _lib.REC_COUNT, fs
    lst.K = _lib.REC_TOPK
    return lst


def _list_of_rows(boxes, lo, n, counts, planes):
    """The _lib.DrawList of rows lo .. lo + n - 1 of dense rows, all contiguous and kept alive by the caller: boxes float32
    [B,K,4|5]; counts: None or int32 [B], the rows of this run that are boxes; planes: {'score': float32 [B,K], 'cls' and
    'id': int64 [B,K]}, entries that are None or missing left out."""
    K, width = boxes.shape[1:]
    lst = _lib.DrawList()
    lst.box, lst.box_frame_stride, lst.box_row_stride = boxes.data_ptr() + 4 * lo * width, K * width, width
    if width == 5:
        lst.angle, lst.angle_frame_stride, lst.angle_row_stride = boxes.data_ptr() + 4 * (lo * width + 4), K * width, width
    for field, size in (('score', 4), ('cls', 8), ('id', 8)):
        if planes.get(field) is not None:
            setattr(lst, field, planes[field].data_ptr() + size * lo)
            setattr(lst, field + '_frame_stride', K)
            setattr(lst, field + '_row_stride', 1)
    if counts is not None:
        lst.count, lst.count_stride = _ptr(counts), 1
    lst.K = n
    return lst


def _launch_on_image(timer_name, image, yuv, rgb_entry, yuv_entry, *tail):
    """One launch of a kernel on the frames or planes of _image: the entry point for packed RGB frames or the one for
    mydet_yuv420_src, each followed by the `tail` arguments and the stream, inside one TIMER span of `timer_name`."""
    t0 = TIMER.start() if TIMER else None
    if yuv is None:
        B, H, W, _ = image.shape
        name = rgb_entry
        code = getattr(_lib.lib(), name)(_ptr(image), B, H, W, image.stride(0), image.stride(1), *tail, _stream())
    else:
        B, H, W = image[0].shape
        name = yuv_entry
        src = _yuv420_src(image, yuv[0], yuv[1], yuv[2])
        code = getattr(_lib.lib(), name)(ctypes.byref(src), B, H, W, *tail, _stream())
    if t0:
        TIMER.stop(timer_name, t0, float(B))
    _lib.check(code, name)


def _draw_launch(image, yuv, lst, style, dev):
    s, keep = style.struct(dev)
    _launch_on_image('draw_boxes', image, yuv, 'mydet_draw_boxes_rgb_u8', 'mydet_draw_boxes_yuv420_u8', ctypes.byref(lst), ctypes.byref(s))
    del keep


def _draw_dense(what, image, yuv, B, boxes, style, counts, scores, classes, ids):
    _draw_check_style(style, what)
    boxes, counts, planes = _box_rows(what, B, boxes, counts, scores, classes, ids)
    dev = _same_device(what, image, [boxes, counts] + list(planes.values()))
    K = boxes.shape[1]
    if K == 0:
        return
    boxes = boxes.contiguous()
    planes = {field: None if planes[name] is None else planes[name].contiguous()
              for field, name in (('score', 'scores'), ('cls', 'classes'), ('id', 'ids'))}
    if counts is not None:
        counts = counts.contiguous()
    step = _lib.DRAW_MAX_BOXES
    for lo in reversed(range(0, K, step)):                           # rows K-1 .. 0 are the paint order: the last chunk first
        n = min(step, K - lo)
        chunk_counts = counts if counts is None or K <= step else (counts - lo).clamp_(0, n).to(torch.int32)
        _draw_launch(image, yuv, _list_of_rows(boxes, lo, n, chunk_counts, planes), style, dev)
        del chunk_counts


def draw_boxes(frames, boxes, style, counts=None, scores=None, classes=None, ids=None):
    """Paint boxes into uint8 RGB frames on the device, IN PLACE, one launch per 512 rows (include/mydet.h:
    mydet_draw_boxes_rgb_u8, where the raster rules are).  frames: [B,H,W,3] or [H,W,3] with packed pixels, any row and frame
    strides (a crop view is drawn in place).  boxes: float32 [B,K,4|5] or [K,4|5], rows (cx, cy, w, h[, degrees]).  counts:
    int32 [B], rows to draw per frame (None: all K; above K means K).  scores float32, classes, ids int64 [B,K]: what labels and
    colours read; None leaves that label part out (colour key 0).  Rows are painted K-1 down to 0, so row 0 ends up on top; more
    than 512 rows go in chunks that keep this order.  style: ops.draw_style(...).  Returns `frames`."""
    what = 'draw_boxes'
    _draw_dense(what, *_image(what, frames, None, None, None, True), boxes, style, counts, scores, classes, ids)
    return frames


def draw_boxes_yuv420(planes, layout, boxes, style, counts=None, scores=None, classes=None, ids=None, matrix='bt601', full_range=False):
    """draw_boxes into the planes of 4:2:0 frames, IN PLACE (include/mydet.h: mydet_draw_boxes_yuv420_u8): layout 'nv12', 'nv21'
    with planes (y [B,H,W], uv [B,ceil(H/2),ceil(W/2),2]), 'i420' with (y, u, v), 'yv12' with (y, v, u); uint8, packed samples,
    any row and frame strides; odd H and W are legal.  'p010' / 'i010' are not drawn into (ValueError).  matrix, full_range:
    how the colours become Y'CbCr (ops.rgb_to_yuv), the selectors of the input side.  Returns `planes`."""
    what = 'draw_boxes_yuv420'
    _draw_dense(what, *_image(what, planes, layout, matrix, full_range, True), boxes, style, counts, scores, classes, ids)
    return planes


def draw_records(target, rec, style, layout=None, matrix='bt601', full_range=False, ids=None):
    """Paint the detections of a record dict (ops.record_views; plain or rotated) into `target`, IN PLACE, in one launch that
    reads the record's planes through their strides -- nothing is copied or synchronised.  target: uint8 RGB frames
    [B,H,W,3] (layout None) or the planes of `layout` as in draw_boxes_yuv420.  The dict must hold views of its 'records'
    buffer (a ValueError for copies, as in track_frames).  ids: optional int64 [B,512].  Returns `target`."""
    what = 'draw_records'
    _draw_check_style(style, what)
    records = _record_buffer(what, rec)
    image, yuv, B = _image(what, target, layout, matrix, full_range, True)
    if B != records.shape[0]:
        raise ValueError(f'{what}: {B} frames and {records.shape[0]} records')
    if ids is not None and (not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64 or tuple(ids.shape) != (B, _lib.REC_TOPK)):
        raise ValueError(f'{what}: ids is an int64 tensor [{B},{_lib.REC_TOPK}]')
    dev = _same_device(what, image, [records, ids])
    ids = None if ids is None else ids.contiguous()
    _draw_launch(image, yuv, _list_of_records(what, records, True, ids), style, dev)
    return target


# ---------------------------------------------------------------------------------------------------------------------------
# Counting overlay and trails (include/mydet.h: mydet_trails_frames, mydet_draw_overlay_rgb_u8 / _yuv420_u8, where the rules are).
# overlay_geometry and overlay_label_text are host functions and ARE the documented rules for ticks, anchors and texts.

OVERLAY_COUNTERS = {'occupancy': _lib.OVERLAY_COUNT_OCCUPANCY, 'entries': _lib.OVERLAY_COUNT_ENTRIES, 'visits': _lib.OVERLAY_COUNT_VISITS}


def trail_set(max_points, anchor='center', classes=None):
    """The parameter struct of mydet_trails_frames (a _lib.TrailSet): max_points 2 .. 32 ring entries per track; anchor 'center'
    or 'bottom' and classes None or 1 .. 16 class indices, as in zone_set.  A ValueError otherwise; touches no device."""
    if isinstance(max_points, bool) or not isinstance(max_points, (int, np.integer)) or not 2 <= max_points <= _lib.TRAIL_MAX_POINTS:
        raise ValueError(f'trail_set: an integer max_points in 2 .. {_lib.TRAIL_MAX_POINTS} expected, got {max_points!r}')
    t = _lib.TrailSet()
    t.max_points, t.anchor = int(max_points), _zone_anchor('trail_set', anchor)
    _set_classes('trail_set', t, classes)
    return t


def trails_state_words(max_tracks, max_points):
    """int32 words of one stream's trail state (include/mydet.h: mydet_trails_state_words); host arithmetic only."""
    max_tracks, max_points = _max_tracks('trails', max_tracks), int(max_points)
    if not 2 <= max_points <= _lib.TRAIL_MAX_POINTS:
        raise ValueError(f'trails: 2 <= max_points <= {_lib.TRAIL_MAX_POINTS} expected, got {max_points}')
    return (max_tracks * (4 + 2 * max_points) + 3) // 4 * 4


_TRAILS_STATE = _StateFamily('trails', 'trails', trails_state_words, 'max_tracks = {}, max_points = {}', 'mydet_trails_reset', _ints, True)


def trails_state(streams, max_tracks, max_points, device):
    """A reset trail state: int32 [streams, trails_state_words(max_tracks, max_points)] (include/mydet.h has the layout)."""
    return _state_new(_TRAILS_STATE, streams, (max_tracks, max_points), device)


def trails_reset_(state, max_tracks, max_points):
    """Reset a trail state in place (mydet_trails_reset): every ring empty."""
    return _state_reset(_TRAILS_STATE, state, (max_tracks, max_points))


def trails_state_views(state, max_tracks, max_points):
    """Field views of a trail state int32 [S, words] (include/mydet.h: mydet_trails_frames), nothing copied: id int64 [S,MT]
    (0 = an empty slot), fill, head int32 [S,MT], ring int32 [S,MT,L,2].  Works on any device (tests read a host copy)."""
    mt, L = int(max_tracks), int(max_points)
    _state_check(_TRAILS_STATE, state, (mt, L), 'trails_state_views', views=True)
    return {'id': state[:, :2 * mt].view(torch.int64), 'fill': state[:, 2 * mt:3 * mt], 'head': state[:, 3 * mt:4 * mt],
            'ring': state[:, 4 * mt:4 * mt + 2 * L * mt].view(state.shape[0], mt, L, 2)}


def trails_frames(track_out, state, trail_set, out=None):
    """Keep the trails of the tracks of S streams x F frames in ONE launch (include/mydet.h: mydet_trails_frames, where the rules
    are).  track_out: the dict ops.track_frames returned.  state: int32 [S, trails_state_words(MT, L)] from trails_state, updated
    in place.  trail_set: trail_set(...).  Returns a dict of int32 device tensors: points [S,F,MT,L,2] (newest first, zeros beyond
    the fill), len [S,F,MT], bbox [S,F,MT,4] (min x, min y, max x, max y), all in 1/16 pixel.  out: such a dict to write into."""
    what = 'trails_frames'
    if not isinstance(trail_set, _lib.TrailSet):
        raise TypeError(f'{what}: trail_set is a _lib.TrailSet (ops.trail_set), got {type(trail_set).__name__}')
    L = trail_set.max_points
    S, F, mt, dev = _track_planes(what, track_out, _TRAILS_STATE, state, L)
    out = out_planes(what, out, {'points': ((S, F, mt, L, 2), torch.int32), 'len': ((S, F, mt), torch.int32),
                                 'bbox': ((S, F, mt, 4), torch.int32)}, dev)
    t0 = TIMER.start() if TIMER else None
    code = _lib.lib().mydet_trails_frames(_ptr(track_out['box']), _ptr(track_out['id']), _ptr(track_out['cls']), _ptr(track_out['missed']),
                                          _ptr(track_out['count']), S, F, mt, ctypes.byref(trail_set), _ptr(state), _ptr(out['points']),
                                          _ptr(out['len']), _ptr(out['bbox']), _stream())
    if t0:
        TIMER.stop('trails_frames', t0, float(S * F))
    _lib.check(code, 'mydet_trails_frames')
    return out


def overlay_counter_flags(counters):
    """The C counter flags of an iterable of 'occupancy' / 'entries' / 'visits' (None or empty: 0 = no labels); a ValueError otherwise."""
    if counters is None:
        return 0
    if isinstance(counters, str):
        counters = (counters,)
    flags = 0
    for name in counters:
        if not isinstance(name, str) or name not in OVERLAY_COUNTERS:
            raise ValueError(f'overlay: counter {name!r} is not one of {sorted(OVERLAY_COUNTERS)}')
        flags |= OVERLAY_COUNTERS[name]
    return flags


def overlay_label_text(name, counters=('occupancy', 'entries'), occupancy=0, entries=0, visits=0, line=None):
    """The text of a counter label (the rule of include/mydet.h as host code).  A zone: `name`, then for each part of `counters`,
    in the order occupancy, entries, visits, a space and `N`, `+E` or `-V`.  A line (line = (pos, neg)): `name +pos -neg`.  A
    number is the decimal of min(value, 999999); the name is cut to 16 characters, the label to 40 glyphs."""
    def num(v):
        return str(min(max(int(v), 0), 999999))
    text = str(name)[:_lib.DRAW_NAME_BYTES]
    if line is not None:
        text += f' +{num(line[0])} -{num(line[1])}'
    else:
        flags = overlay_counter_flags(counters)
        if flags & _lib.OVERLAY_COUNT_OCCUPANCY:
            text += f' {num(occupancy)}'
        if flags & _lib.OVERLAY_COUNT_ENTRIES:
            text += f' +{num(entries)}'
        if flags & _lib.OVERLAY_COUNT_VISITS:
            text += f' -{num(visits)}'
    return text[:_lib.OVERLAY_MAX_GLYPHS]


def overlay_tick(line, thickness):
    """The direction tick (M.x, M.y, E.x, E.y) of a quantised line (A.x, A.y, B.x, B.y), by integers alone (include/mydet.h):
    M = (A + B) >> 1; n = (-(B.y - A.y), B.x - A.x); E = M + trunc(n * 16 * 4 * thickness / isqrt(len2))."""
    ax, ay, bx, by = (int(v) for v in line)
    mx, my = (ax + bx) >> 1, (ay + by) >> 1
    nx, ny = -(by - ay), bx - ax
    lh = math.isqrt(nx * nx + ny * ny)
    k = 16 * 4 * int(thickness)

    def trunc_div(v):
        return (abs(v) // lh) * (1 if v >= 0 else -1)
    return mx, my, mx + trunc_div(nx * k), my + trunc_div(ny * k)


class OverlayGeometry:
    """What ops.overlay_geometry returns: the static geometry of the overlay on the host (`struct`, a _lib.OverlayGeometry, with
    n_polygons, n_lines and thickness); its device buffer is made the first time a device paints with it."""

    def __init__(self, struct, n_polygons, n_lines, thickness):
        self.struct, self.n_polygons, self.n_lines, self.thickness = struct, n_polygons, n_lines, thickness
        self._buffers = {}

    def __repr__(self):
        return f'OverlayGeometry({self.n_polygons} polygons, {self.n_lines} lines, thickness={self.thickness})'

    def buffer(self, device):
        key = str(torch.device(device))
        if key not in self._buffers:
            raw = np.frombuffer(bytes(self.struct), dtype=np.uint8).copy()
            self._buffers[key] = torch.from_numpy(raw).to(device)
        return self._buffers[key]


def overlay_geometry(zone_set, names=None, thickness=2):
    """The host part of the overlay painter (include/mydet.h: mydet_overlay_geometry): the quantised polygons and lines of a
    zone_set(...), the direction tick of every line (overlay_tick; it depends on `thickness`, 1 .. 64, the thickness of outlines,
    lines and ticks), the label anchors -- a zone's vertex least in (y, x), a line's midpoint -- and the names (one per polygon
    followed by one per line, 16 ASCII characters are shown; None: zone0 .. and line0 ..).  Touches no device."""
    if not isinstance(zone_set, _lib.ZoneSet):
        raise TypeError(f'overlay_geometry: zone_set is a _lib.ZoneSet (ops.zone_set), got {type(zone_set).__name__}')
    if isinstance(thickness, bool) or not isinstance(thickness, (int, np.integer)) or not 1 <= thickness <= _lib.DRAW_MAX_THICKNESS:
        raise ValueError(f'overlay_geometry: an integer thickness in 1..{_lib.DRAW_MAX_THICKNESS} expected, got {thickness!r}')
    Z, L = zone_set.n_polygons, zone_set.n_lines
    if names is None:
        names = [f'zone{z}' for z in range(Z)] + [f'line{l}' for l in range(L)]
    names = list(names)
    if len(names) != Z + L or not all(isinstance(n, str) for n in names):
        raise ValueError(f'overlay_geometry: names is one str per polygon followed by one per line ({Z + L}), got {names!r}')
    g = _lib.OverlayGeometry()
    for z in range(Z):
        n = zone_set.n_vertices[z]
        g.n_vertices[z] = n
        pts = [(zone_set.polygon[z][i][0], zone_set.polygon[z][i][1]) for i in range(n)]
        for i, (x, y) in enumerate(pts):
            g.polygon[z][i][0], g.polygon[z][i][1] = x, y
        y, x = min((y, x) for x, y in pts)
        g.anchor[z][0], g.anchor[z][1] = x, y
    for l in range(L):
        line = list(zone_set.line[l])
        g.line[l][:] = line
        tick = overlay_tick(line, thickness)
        g.tick[l][:] = list(tick)
        g.anchor[_lib.ZONES_MAX + l][0], g.anchor[_lib.ZONES_MAX + l][1] = tick[0], tick[1]
    for k, name in enumerate(names):
        raw = name.encode('ascii', 'replace')[:_lib.DRAW_NAME_BYTES]
        slot = k if k < Z else _lib.ZONES_MAX + k - Z
        g.name[slot][:len(raw)] = list(raw)
    return OverlayGeometry(g, Z, L, int(thickness))


def _overlay_alpha(what, name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= 255:
        raise ValueError(f'{what}: an integer {name} in 0..255 expected, got {v!r}')
    return int(v)


def _overlay_struct(what, B, geometry, zones_out, trails_out, track_out, zones, lines, counters, zone_alpha, occupied_alpha,
                    trail_thickness, coasting):
    """The checked _lib.Overlay of a draw_overlay call and the tensors it points to."""
    o = _lib.Overlay()
    o.zone_alpha, o.occupied_alpha = _overlay_alpha(what, 'zone_alpha', zone_alpha), _overlay_alpha(what, 'occupied_alpha', occupied_alpha)
    if isinstance(trail_thickness, bool) or not isinstance(trail_thickness, (int, np.integer)) or not 1 <= trail_thickness <= _lib.DRAW_MAX_THICKNESS:
        raise ValueError(f'{what}: an integer trail_thickness in 1..{_lib.DRAW_MAX_THICKNESS} expected, got {trail_thickness!r}')
    o.trail_thickness, o.thickness, o.coasting = int(trail_thickness), 1, int(bool(coasting))
    keep, shape = [], None
    if geometry is not None:
        if not isinstance(geometry, OverlayGeometry):
            raise TypeError(f'{what}: geometry is an ops.OverlayGeometry (ops.overlay_geometry), got {type(geometry).__name__}')
        Z, L = geometry.n_polygons, geometry.n_lines
        paint_z, paint_l = bool(zones) and Z > 0, bool(lines) and L > 0
        o.counters = overlay_counter_flags(counters)
        if paint_z or paint_l:
            if not isinstance(zones_out, dict):
                raise ValueError(f'{what}: zones_out, the dict of ops.zones_frames on the same zone_set, is needed to paint zones or lines')
            S, F = zones_out['occupancy'].shape[:2] if Z else zones_out['line_counts'].shape[:2]
            shape = (int(S), int(F))
            for k, want in (('occupancy', (S, F, Z)), ('zone_counts', (S, F, Z, 4)), ('line_counts', (S, F, L, 2))):
                t = zones_out[k]
                if not isinstance(t, torch.Tensor) or tuple(t.shape) != want or t.dtype != torch.int32 or not t.is_contiguous():
                    raise ValueError(f'{what}: zones_out[{k!r}] must be a contiguous int32 tensor {want}')
                keep.append(t)
            o.flags |= (_lib.OVERLAY_ZONES if paint_z else 0) | (_lib.OVERLAY_LINES if paint_l else 0)
            o.n_polygons, o.n_lines, o.thickness = Z, L, geometry.thickness
            o.occupancy, o.zone_counts, o.line_counts = (_ptr(t) if t.numel() else None for t in keep)
    if trails_out is not None:
        if not isinstance(trails_out, dict) or not isinstance(track_out, dict):
            raise ValueError(f'{what}: trails_out is the dict of ops.trails_frames and needs track_out, the dict of ops.track_frames it was made from')
        pts = trails_out['points']
        if not isinstance(pts, torch.Tensor) or pts.dim() != 5 or pts.shape[4] != 2:
            raise ValueError(f'{what}: trails_out is the dict of ops.trails_frames (points [S,F,MT,L,2], len, bbox)')
        S, F, mt, L = (int(v) for v in pts.shape[:4])
        if shape is not None and shape != (S, F):
            raise ValueError(f'{what}: zones_out is of {shape[0]} x {shape[1]} frames, trails_out of {S} x {F}')
        shape = (S, F)
        wants = (('points', trails_out, (S, F, mt, L, 2), torch.int32), ('len', trails_out, (S, F, mt), torch.int32),
                 ('bbox', trails_out, (S, F, mt, 4), torch.int32), ('id', track_out, (S, F, mt), torch.int64),
                 ('missed', track_out, (S, F, mt), torch.int32))
        for k, src, want, dt in wants:
            t = src[k]
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != want or t.dtype != dt or not t.is_contiguous():
                raise ValueError(f'{what}: {k!r} must be a contiguous {dt} tensor {want}')
            keep.append(t)
        if not (1 <= mt <= _lib.TRACK_MAX_TRACKS and 2 <= L <= _lib.TRAIL_MAX_POINTS):
            raise ValueError(f'{what}: trails of 1..{_lib.TRACK_MAX_TRACKS} tracks and 2..{_lib.TRAIL_MAX_POINTS} points expected, got {mt} and {L}')
        o.flags |= _lib.OVERLAY_TRAILS
        o.max_tracks, o.max_points = mt, L
        o.trail_points, o.trail_len, o.trail_bbox, o.id, o.missed = (_ptr(t) for t in keep[-5:])
    if not o.flags:
        raise ValueError(f'{what}: nothing to paint: neither zones or lines of a geometry nor trails')
    if shape[0] * shape[1] != B:
        raise ValueError(f'{what}: {B} frames, but the counting outputs are of {shape[0]} streams x {shape[1]} frames')
    o.S, o.F = shape
    return o, keep


def _draw_overlay(what, image, yuv, B, style, kwargs):
    _draw_check_style(style, what)
    o, keep = _overlay_struct(what, B, **kwargs)                     # every argument rule, before a device is touched
    dev = _same_device(what, image, keep)
    if o.flags & (_lib.OVERLAY_ZONES | _lib.OVERLAY_LINES):
        keep.append(kwargs['geometry'].buffer(dev))
        o.geometry = _ptr(keep[-1])
    s, keep_style = style.struct(dev)
    if o.counters and (o.flags & (_lib.OVERLAY_ZONES | _lib.OVERLAY_LINES)) and not s.atlas:
        atlas = glyph_atlas(style.label_height, dev)
        s.atlas, s.ch, s.cw = _ptr(atlas), atlas.shape[1], atlas.shape[2]
    _launch_on_image('draw_overlay', image, yuv, 'mydet_draw_overlay_rgb_u8', 'mydet_draw_overlay_yuv420_u8', ctypes.byref(o), ctypes.byref(s))
    del keep, keep_style


def draw_overlay(frames, style, geometry=None, zones_out=None, trails_out=None, track_out=None, zones=True, lines=True,
                 counters=('occupancy', 'entries'), zone_alpha=48, occupied_alpha=96, trail_thickness=2, coasting=False):
    """Paint the counting overlay into uint8 RGB frames on the device, IN PLACE, in one launch (include/mydet.h:
    mydet_draw_overlay_rgb_u8, where the raster rules are).  frames: as in draw_boxes, [S*F,H,W,3] in the frame order of the
    counting outputs.  style: ops.draw_style(...): its palette and, for the counter labels, its label_height are used.
    geometry: overlay_geometry(...) of the zone_set that made zones_out, the dict of ops.zones_frames (occupancy, zone_counts,
    line_counts are read on the device); zones / lines: paint the polygons (fill, outline) / the lines with their ticks;
    counters: the parts of a zone's label, any of 'occupancy', 'entries', 'visits' (empty: no labels, of lines neither).
    trails_out: the dict of ops.trails_frames, painted with trail_thickness for the tracks of track_out (the dict of
    ops.track_frames both were made from) that the call shows: missed == 0, with coasting=True every live track.  Returns `frames`."""
    what = 'draw_overlay'
    kwargs = dict(geometry=geometry, zones_out=zones_out, trails_out=trails_out, track_out=track_out, zones=zones, lines=lines, counters=counters,
                  zone_alpha=zone_alpha, occupied_alpha=occupied_alpha, trail_thickness=trail_thickness, coasting=coasting)
    _draw_overlay(what, *_image(what, frames, None, None, None, True), style, kwargs)
    return frames


def draw_overlay_yuv420(planes, layout, style, geometry=None, zones_out=None, trails_out=None, track_out=None, zones=True, lines=True,
                        counters=('occupancy', 'entries'), zone_alpha=48, occupied_alpha=96, trail_thickness=2, coasting=False,
                        matrix='bt601', full_range=False):
    """draw_overlay into the planes of 4:2:0 frames, IN PLACE (include/mydet.h: mydet_draw_overlay_yuv420_u8); planes, layout,
    matrix and full_range as in draw_boxes_yuv420 ('p010' / 'i010' are not drawn into: ValueError).  Returns `planes`."""
    what = 'draw_overlay_yuv420'
    kwargs = dict(geometry=geometry, zones_out=zones_out, trails_out=trails_out, track_out=track_out, zones=zones, lines=lines, counters=counters,
                  zone_alpha=zone_alpha, occupied_alpha=occupied_alpha, trail_thickness=trail_thickness, coasting=coasting)
    _draw_overlay(what, *_image(what, planes, layout, matrix, full_range, True), style, kwargs)
    return planes


# ---------------------------------------------------------------------------------------------------------------------------
# Redaction (include/mydet.h: mydet_redact_boxes_rgb_u8 / mydet_redact_boxes_yuv420_u8, where the rules are).

REDACT_MODES = {'mosaic': _lib.REDACT_MOSAIC, 'smooth': _lib.REDACT_SMOOTH, 'solid': _lib.REDACT_SOLID}
REDACT_SHAPES = {'box': _lib.REDACT_BOX, 'ellipse': _lib.REDACT_ELLIPSE}
_REDACT_WS = {}


class RedactStyle:
    """What ops.redact_style returns: the checked settings of a redaction, on the host."""

    def __init__(self, mode, cell, shape, pad, classes, color):
        self.mode, self.cell, self.shape, self.pad, self.classes, self.color = mode, cell, shape, pad, classes, color

    def __repr__(self):
        return (f'RedactStyle(mode={self.mode!r}, cell={self.cell}, shape={self.shape!r}, pad={self.pad}, classes={self.classes}, '
                f'color={self.color})')

    def struct(self):
        """The mydet_redact_style."""
        s = _lib.RedactStyle()
        s.mode, s.shape, s.cell, s.pad = REDACT_MODES[self.mode], REDACT_SHAPES[self.shape], self.cell, self.pad
        s.color[0], s.color[1], s.color[2] = self.color
        s.n_classes = len(self.classes or ())
        for k, c in enumerate(self.classes or ()):
            s.classes[k] = c
        return s


def redact_style(mode='mosaic', cell=16, shape='box', pad=1.0, classes=None, color=(0, 0, 0)):
    """The settings of a redaction, checked here and touching no device (a RedactStyle; include/mydet.h has the rules).  mode:
    'mosaic' (a covered pixel becomes the mean of its cell), 'smooth' (the bilinear interpolation of the cell means: a strong
    blur) or 'solid' (`color`).  cell: the cell size, even, 4..64.  shape: 'box' or 'ellipse', what of a row is covered.  pad:
    the row is scaled by it first, finite and > 0.  classes: None = every row, or 1..16 class indices = only rows of these.
    color: the (r, g, b) of 'solid'."""
    if not isinstance(mode, str) or mode not in REDACT_MODES:
        raise ValueError(f'redact_style: mode {mode!r} is not one of {sorted(REDACT_MODES)}')
    if not isinstance(shape, str) or shape not in REDACT_SHAPES:
        raise ValueError(f'redact_style: shape {shape!r} is not one of {sorted(REDACT_SHAPES)}')
    if isinstance(cell, bool) or not isinstance(cell, int) or not _lib.REDACT_MIN_CELL <= cell <= _lib.REDACT_MAX_CELL or cell % 2:
        raise ValueError(f'redact_style: an even integer cell in {_lib.REDACT_MIN_CELL}..{_lib.REDACT_MAX_CELL} expected, got {cell!r}')
    try:
        pad = float(pad)
    except (TypeError, ValueError):
        raise ValueError(f'redact_style: pad is a finite number > 0, got {pad!r}') from None
    if not (math.isfinite(pad) and pad > 0) or float(np.float32(pad)) <= 0 or not math.isfinite(float(np.float32(pad))):
        raise ValueError(f'redact_style: pad is a finite number > 0, got {pad!r}')
    if classes is not None:
        try:
            ok = all(isinstance(c, (int, np.integer)) and not isinstance(c, bool) for c in classes)
            classes = tuple(int(c) for c in classes) if ok else None
        except TypeError:
            classes = None
        if classes is None or not 1 <= len(classes) <= _lib.REDACT_MAX_CLASSES or any(not -2 ** 31 <= c < 2 ** 31 for c in classes):
            raise ValueError(f'redact_style: classes is None or 1..{_lib.REDACT_MAX_CLASSES} class indices')
    try:
        color = tuple(int(v) for v in color)
    except (TypeError, ValueError):
        raise ValueError(f'redact_style: color = (r, g, b) expected, got {color!r}') from None
    if len(color) != 3 or min(color) < 0 or max(color) > 255:
        raise ValueError(f'redact_style: color = (r, g, b) with entries in 0..255 expected, got {color!r}')
    return RedactStyle(mode, cell, shape, pad, classes, color)


def _redact_check_style(style, what):
    if not isinstance(style, RedactStyle):
        raise TypeError(f'{what}: style is an ops.RedactStyle (ops.redact_style), got {type(style).__name__}')


def _redact_launch(image, yuv, lst, style, dev):
    """The two kernels of one redaction, one TIMER span; the means workspace is kept per (device, B, H, W, cell)."""
    B, H, W = (image.shape if yuv is None else image[0].shape)[:3]
    ws = None
    if style.mode != 'solid':
        key = (dev, B, H, W, style.cell)
        if key not in _REDACT_WS:
            _REDACT_WS[key] = torch.empty(_lib.lib().mydet_redact_workspace_bytes(B, H, W, style.cell) // 4, dtype=torch.int32, device=dev)
        ws = _REDACT_WS[key]
    s = style.struct()
    _launch_on_image('redact_boxes', image, yuv, 'mydet_redact_boxes_rgb_u8', 'mydet_redact_boxes_yuv420_u8', ctypes.byref(lst), ctypes.byref(s),
                     _ptr(ws))


def _redact_dense(what, image, yuv, B, boxes, style, counts, classes):
    _redact_check_style(style, what)
    boxes, counts, planes = _box_rows(what, B, boxes, counts, None, classes, None)
    if style.classes is not None and planes['classes'] is None:
        raise ValueError(f'{what}: a style with a class filter needs classes')
    K = boxes.shape[1]
    if K > _lib.DRAW_MAX_BOXES:
        raise ValueError(f'{what}: at most {_lib.DRAW_MAX_BOXES} rows per frame are redacted in one call (every new value comes from the '
                         f'original frame), got {K}')
    dev = _same_device(what, image, [boxes, counts, planes['classes']])
    if K == 0:
        return
    boxes = boxes.contiguous()
    counts = None if counts is None else counts.contiguous()
    cls = planes['classes'].contiguous() if style.classes is not None else None
    _redact_launch(image, yuv, _list_of_rows(boxes, 0, K, counts, {'cls': cls}), style, dev)


def redact_boxes(frames, boxes, style, counts=None, classes=None):
    """Hide boxes in uint8 RGB frames on the device, IN PLACE: mosaic, smooth blur or one colour (include/mydet.h:
    mydet_redact_boxes_rgb_u8, where the rules are).  frames: [B,H,W,3] or [H,W,3] with packed pixels, any row and frame
    strides (a crop view is redacted in place).  boxes: float32 [B,K,4|5] or [K,4|5], rows (cx, cy, w, h[, degrees]), K <= 512.
    counts: int32 [B], the rows of each frame that are boxes (None: all K; above K means K).  classes: int64 [B,K], what a
    style with a class filter reads.  Every new value is a function of the original frame: row order and overlaps do not
    matter.  style: ops.redact_style(...).  Returns `frames`."""
    what = 'redact_boxes'
    _redact_dense(what, *_image(what, frames, None, None, None, True), boxes, style, counts, classes)
    return frames


def redact_boxes_yuv420(planes, layout, boxes, style, counts=None, classes=None, matrix='bt601', full_range=False):
    """redact_boxes in the planes of 4:2:0 frames, IN PLACE (include/mydet.h: mydet_redact_boxes_yuv420_u8): planes, layout as
    in draw_boxes_yuv420 ('nv12', 'nv21', 'i420', 'yv12'; odd H and W are legal; 'p010' / 'i010' give a ValueError).  matrix,
    full_range: how the colour of 'solid' becomes Y'CbCr (ops.rgb_to_yuv).  Returns `planes`."""
    what = 'redact_boxes_yuv420'
    _redact_dense(what, *_image(what, planes, layout, matrix, full_range, True), boxes, style, counts, classes)
    return planes


def redact_records(target, rec, style, layout=None, matrix='bt601', full_range=False):
    """Hide the detections of a record dict (ops.record_views; plain or rotated) in `target`, IN PLACE, reading the record's
    planes through their strides -- nothing is copied or synchronised.  target: uint8 RGB frames [B,H,W,3] (layout None) or
    the planes of `layout` as in redact_boxes_yuv420.  The dict must hold views of its 'records' buffer (a ValueError for
    copies, as in draw_records).  Returns `target`."""
    what = 'redact_records'
    _redact_check_style(style, what)
    records = _record_buffer(what, rec)
    image, yuv, B = _image(what, target, layout, matrix, full_range, True)
    if B != records.shape[0]:
        raise ValueError(f'{what}: {B} frames and {records.shape[0]} records')
    dev = _same_device(what, image, [records])
    _redact_launch(image, yuv, _list_of_records(what, records, style.classes is not None, None), style, dev)
    return target


# ---------------------------------------------------------------------------------------------------------------------------
# Object chips (include/mydet.h: mydet_crop_boxes_rgb / mydet_crop_boxes_yuv420, where the sampling rules are).

CROP_OUTPUTS = ('uint8', 'input')


def crop_settings(what, size, max_per_frame, pad, fill, out, input_format):
    """The checked settings of a crop call (no device touched): ((ch, cw), M or None, pad, (r, g, b), float output?, input format).
    size = (height, width), each 1..256; max_per_frame None or 1..512; pad finite and > 0; fill three integers 0..255; out 'uint8'
    or 'input' (float32 chips in the arithmetic of preprocess_u8 for input_format 'RGB_1' (None) or 'RGB_1_norm')."""
    try:
        ch, cw = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f'{what}: size = (height, width) expected, got {size!r}') from None
    if not (1 <= ch <= _lib.CROP_MAX_SIDE and 1 <= cw <= _lib.CROP_MAX_SIDE):
        raise ValueError(f'{what}: size = (height, width) with entries in 1..{_lib.CROP_MAX_SIDE} expected, got {size!r}')
    if max_per_frame is not None:
        if isinstance(max_per_frame, bool) or not isinstance(max_per_frame, int) or not 1 <= max_per_frame <= _lib.CROP_MAX_SLOTS:
            raise ValueError(f'{what}: max_per_frame is None or an int in 1..{_lib.CROP_MAX_SLOTS}, got {max_per_frame!r}')
    pad = float(pad)
    if not (math.isfinite(pad) and pad > 0) or float(np.float32(pad)) <= 0 or not math.isfinite(float(np.float32(pad))):
        raise ValueError(f'{what}: pad is a finite number > 0, got {pad!r}')
    try:
        fill = tuple(int(v) for v in fill)
    except (TypeError, ValueError):
        raise ValueError(f'{what}: fill = (r, g, b) expected, got {fill!r}') from None
    if len(fill) != 3 or min(fill) < 0 or max(fill) > 255:
        raise ValueError(f'{what}: fill = (r, g, b) with entries in 0..255 expected, got {fill!r}')
    if not isinstance(out, str) or out not in CROP_OUTPUTS:
        raise ValueError(f'{what}: out {out!r} is not one of {CROP_OUTPUTS}')
    input_format = 'RGB_1' if input_format is None else input_format
    if input_format not in ('RGB_1', 'RGB_1_norm'):
        raise ValueError(f"{what}: input_format {input_format!r} is not 'RGB_1' or 'RGB_1_norm'")
    return (ch, cw), max_per_frame, pad, fill, out == 'input', input_format


def _crop_dst(what, dst, B, M, chip, f32, dev):
    """The chip tensor: zeros when dst is None; else dst checked -- [B,M,ch,cw,3] uint8 or [B,M,3,ch,cw] float32 on `dev`, every
    chip contiguous, any non-negative slot and frame strides."""
    ch, cw = chip
    shape = (B, M, 3, ch, cw) if f32 else (B, M, ch, cw, 3)
    dtype = torch.float32 if f32 else torch.uint8
    if dst is None:
        return torch.zeros(shape, dtype=dtype, device=dev)
    if not isinstance(dst, torch.Tensor) or dst.dtype != dtype:
        raise TypeError(f'{what}: dst is a {dtype} tensor, got {dst.dtype if isinstance(dst, torch.Tensor) else type(dst).__name__}')
    if tuple(dst.shape) != shape:
        raise ValueError(f'{what}: dst of shape {shape} expected, got {tuple(dst.shape)}')
    if dst.device != dev:
        raise ValueError(f'{what}: the source is on {dev}, dst on {dst.device}')
    if M and (not dst[0, 0].is_contiguous() or dst.stride(1) < 3 * ch * cw or dst.stride(0) < 0):
        raise ValueError(f'{what}: dst needs contiguous chips (strides {tuple(dst.stride())} of {tuple(dst.shape)})')
    return dst


def _crop_launch(image, yuv, lst, settings, M, dst):
    chip, _, pad, fill, f32, input_format = settings
    o = _lib.CropOut()
    o.ch, o.cw, o.M, o.kind, o.pad = chip[0], chip[1], M, _lib.CROP_F32 if f32 else _lib.CROP_U8, pad
    o.fill[0], o.fill[1], o.fill[2] = fill
    o.norm, o.mean3, o.std3 = _norm_args(input_format)
    o.out, o.slot_stride, o.frame_stride = dst.data_ptr(), dst.stride(1), dst.stride(0)
    _launch_on_image('crop_boxes', image, yuv, 'mydet_crop_boxes_rgb', 'mydet_crop_boxes_yuv420', ctypes.byref(lst), ctypes.byref(o))


def _crop_dense(what, image, yuv, B, boxes, settings, counts, dst):
    boxes, counts, _ = _box_rows(what, B, boxes, counts, None, None, None)
    dev = _same_device(what, image, [boxes, counts])
    K = min(boxes.shape[1], _lib.DRAW_MAX_BOXES)                     # rows past the launch's 512 get no chip
    M = settings[1] if settings[1] is not None else K
    dst = _crop_dst(what, dst, B, M, settings[0], settings[4], dev)
    if K == 0 or M == 0:
        return dst
    boxes = boxes.contiguous()
    counts = None if counts is None else counts.contiguous()
    _crop_launch(image, yuv, _list_of_rows(boxes, 0, K, counts, {}), settings, M, dst)
    return dst


def crop_boxes(frames, boxes, size, counts=None, max_per_frame=None, pad=1.0, fill=(0, 0, 0), out='uint8', input_format=None, dst=None):
    """The chips of boxes: every box cut out of uint8 RGB frames on the device, turned upright and resampled to size = (height,
    width), in ONE launch (include/mydet.h: mydet_crop_boxes_rgb, where the sampling rules are).  frames: [B,H,W,3] or [H,W,3],
    read in place through their strides when pixels are packed (a crop view is read in place).  boxes: float32 [B,K,4|5] or
    [K,4|5], rows (cx, cy, w, h[, degrees]) in frame pixels; of more than 512 rows the first 512 are read.  counts: int32 [B],
    the rows of each frame that are boxes (None: all K).  max_per_frame: the chip slots M per frame (None: K); a frame gets the
    chips of its first min(count, K, M) rows.  pad: the box is scaled by it first (1.2 = 20 % context).  fill: the (r, g, b) of
    everything outside the frame and of rows that are not boxes (non-finite, w <= 0 or h <= 0).  out: 'uint8' gives
    [B,M,ch,cw,3] uint8; 'input' gives [B,M,3,ch,cw] float32, value / 255 and, with input_format 'RGB_1_norm', the ImageNet
    normalisation -- the arithmetic of preprocess_u8.  dst: an optional tensor of that shape to write into (contiguous chips,
    any slot and frame strides): only chips m < min(count, K, M) are written; without it the chips are new and the others zero."""
    what = 'crop_boxes'
    settings = crop_settings(what, size, max_per_frame, pad, fill, out, input_format)
    return _crop_dense(what, *_image(what, frames, None, None, None, False), boxes, settings, counts, dst)


def crop_boxes_yuv420(planes, layout, boxes, size, counts=None, max_per_frame=None, pad=1.0, fill=(0, 0, 0), out='uint8', input_format=None,
                      dst=None, matrix='bt601', full_range=False):
    """crop_boxes out of 4:2:0 frames (include/mydet.h: mydet_crop_boxes_yuv420): the bits of crop_boxes on
    yuv420_to_rgb(planes, layout, matrix, full_range), which is never built.  planes, layout, matrix, full_range as in
    yuv420_to_rgb: every layout, the 10-bit ones included, odd H and W.  fill is an RGB colour."""
    what = 'crop_boxes_yuv420'
    settings = crop_settings(what, size, max_per_frame, pad, fill, out, input_format)
    return _crop_dense(what, *_image(what, planes, layout, matrix, full_range, False), boxes, settings, counts, dst)


def crop_records(source, rec, size, layout=None, max_per_frame=None, pad=1.0, fill=(0, 0, 0), out='uint8', input_format=None, dst=None,
                 matrix='bt601', full_range=False):
    """The chips of the detections of a record dict (ops.record_views; plain or rotated) in ONE launch that reads the record's
    planes in place through their strides -- nothing is copied or synchronised.  source: uint8 RGB frames [B,H,W,3] (layout
    None) or the planes of `layout` as in crop_boxes_yuv420.  The dict must hold views of its 'records' buffer (a ValueError
    for copies, as in draw_records).  max_per_frame: chip slots per frame (None: 512); chip m of frame b shows the record's row
    m.  Everything else as in crop_boxes."""
    what = 'crop_records'
    settings = crop_settings(what, size, max_per_frame, pad, fill, out, input_format)
    records = _record_buffer(what, rec)
    image, yuv, B = _image(what, source, layout, matrix, full_range, False)
    if B != records.shape[0]:
        raise ValueError(f'{what}: {B} frames and {records.shape[0]} records')
    dev = _same_device(what, image, [records])
    M = settings[1] if settings[1] is not None else _lib.REC_TOPK
    dst = _crop_dst(what, dst, B, M, settings[0], settings[4], dev)
    _crop_launch(image, yuv, _list_of_records(what, records, False, None), settings, M, dst)
    return dst


# --------------------------------------------------------------------------------------------------------------------------
# Appearance (include/mydet.h: mydet_appear_boxes_rgb_u8 and mydet_track_frames_appear_f32 have the rules): a 128-bin colour
# descriptor per box, and the settings and state of the tracker's gate, re-identification and templates.

def _appear_level(what, name, v):
    """A fraction of the largest similarity -> the integer scale of S: floor(v * 131072 + 0.5); None and 0 are 0 = off."""
    if v is None:
        return 0
    v = float(v)
    if not 0 <= v <= 1:                                                # false for a NaN
        raise ValueError(f'{what}: {name} is None (off) or a fraction in [0, 1] of the largest similarity, got {v!r}')
    return int(math.floor(v * _lib.APPEAR_SIM_MAX + 0.5))


def appear_set(gate=0.3, reid=0.6, momentum=0.9, reach=2.0, update_thres=0.3):
    """The appearance settings of mydet_track_frames_appear_f32 (a _lib.TrackAppear).  gate, reid: None or 0 (off), or a fraction
    in (0, 1] of the largest similarity, converted to the integer scale of S by floor(v * 131072 + 0.5).  momentum in [0, 1): the
    share of the old template a match keeps; alpha = floor((1 - momentum) * 256 + 0.5) must land in 1..256.  reach: finite, >= 0.
    update_thres: the detection score from which a match moves the template (not NaN).  ValueError for anything out of range;
    touches no device."""
    what = 'appear_set'
    a = _lib.TrackAppear()
    a.gate, a.reid = _appear_level(what, 'gate', gate), _appear_level(what, 'reid', reid)
    m = float(momentum)
    alpha = int(math.floor((1.0 - m) * 256 + 0.5)) if 0 <= m <= 1 else 0
    if not 1 <= alpha <= 256:
        raise ValueError(f'{what}: momentum in [0, 1) with (1 - momentum) * 256 rounding to 1..256 expected, got {momentum!r}')
    a.alpha = alpha
    r, u = float(reach), float(update_thres)
    if not (math.isfinite(r) and r >= 0 and math.isfinite(float(np.float32(r)))):
        raise ValueError(f'{what}: reach is a finite number >= 0, got {reach!r}')
    if math.isnan(u):
        raise ValueError(f'{what}: update_thres is a number, got {update_thres!r}')
    a.reach, a.update_thres = r, u
    return a


def appear_state_words(max_tracks):
    """int32 words of one stream's appearance state (mydet_track_appear_state_words); host arithmetic only."""
    return ((1 + _lib.APPEAR_BINS) * _max_tracks('tracker', max_tracks) + 3) // 4 * 4


# the one family whose state may live on the host: its reset is a fill, and nothing but the tracker launch reads it
_APPEAR_STATE = _StateFamily('appear', 'appear_state', appear_state_words, 'the appearance templates of max_tracks = {}', None, None, False)


def appear_state(streams, max_tracks, device):
    """A cleared appearance state: int32 zeros [streams, appear_state_words(max_tracks)] -- no slot has a template."""
    return _state_new(_APPEAR_STATE, streams, (max_tracks,), device)


def appear_reset_(state, max_tracks):
    """Clear an appearance state in place: every `has` flag and every template bin is 0 (the state's initial value)."""
    return _state_reset(_APPEAR_STATE, state, (max_tracks,))


def appear_ws_words(max_tracks):
    """int32 words of one stream's similarity workspace (mydet_track_appear_ws_words): 512 * max_tracks; host arithmetic only."""
    return _lib.REC_TOPK * _max_tracks('tracker', max_tracks)


def appear_workspace(streams, max_tracks, device):
    """The workspace of the fused cost (track_frames' appear_ws): int32 [streams, appear_ws_words(max_tracks)], not initialised
    -- the launch assumes nothing about its content."""
    words = appear_ws_words(max_tracks)
    return torch.empty((check_streams('appear_workspace', streams), words), dtype=torch.int32, device=device)


def _workspace_check(ws, S, mt, dev, what):
    words = appear_ws_words(mt)
    if (not isinstance(ws, torch.Tensor) or ws.dtype != torch.int32 or tuple(ws.shape) != (S, words) or ws.device != dev or
            not ws.is_contiguous()):
        got = f'{ws.dtype} {tuple(ws.shape)} on {ws.device}' if isinstance(ws, torch.Tensor) else type(ws).__name__
        raise ValueError(f'{what}: appear_ws must be the contiguous int32 [{S}, {words}] tensor of ops.appear_workspace on {dev}, got {got}')


def appear_state_views(state, max_tracks):
    """Field views of an appearance state int32 [S, words], nothing copied: has int32 [S,MT], tmpl int32 [S,128,MT] in units of
    1/256 sample (bin-major).  Works on any device."""
    _state_check(_APPEAR_STATE, state, (max_tracks,), 'appear_state_views', views=True)
    mt = int(max_tracks)
    return {'has': state[:, :mt], 'tmpl': state[:, mt:mt + _lib.APPEAR_BINS * mt].view(state.shape[0], _lib.APPEAR_BINS, mt)}


def _appear_out(what, out, B, K, dev):
    shape = (B, K, _lib.APPEAR_BINS)
    if out is None:
        return torch.empty(shape, dtype=torch.uint16, device=dev)
    if not isinstance(out, torch.Tensor) or out.dtype != torch.uint16:
        raise TypeError(f'{what}: out is a uint16 tensor, got {out.dtype if isinstance(out, torch.Tensor) else type(out).__name__}')
    if tuple(out.shape) != shape or out.device != dev:
        raise ValueError(f'{what}: out of shape {shape} on {dev} expected, got {tuple(out.shape)} on {out.device}')
    if K and (not out[0].is_contiguous() or out.stride(0) % 2 or out.stride(0) < K * _lib.APPEAR_BINS or out.data_ptr() % 4):
        raise ValueError(f'{what}: out needs contiguous frames, an even frame stride and a 4-byte aligned base (strides {tuple(out.stride())})')
    return out


def _appear_launch(image, yuv, lst, desc):
    _launch_on_image('appear_boxes', image, yuv, 'mydet_appear_boxes_rgb_u8', 'mydet_appear_boxes_yuv420', ctypes.byref(lst), desc.data_ptr(),
                     desc.stride(0))


def _appear_dense(what, image, yuv, B, boxes, counts, out):
    boxes, counts, _ = _box_rows(what, B, boxes, counts, None, None, None)
    if boxes.shape[1] > _lib.DRAW_MAX_BOXES:
        raise ValueError(f'{what}: at most {_lib.DRAW_MAX_BOXES} rows per frame and launch, got {boxes.shape[1]}')
    dev = _same_device(what, image, [boxes, counts])
    K = boxes.shape[1]
    desc = _appear_out(what, out, B, K, dev)
    if K == 0:
        return desc
    boxes = boxes.contiguous()
    counts = None if counts is None else counts.contiguous()
    _appear_launch(image, yuv, _list_of_rows(boxes, 0, K, counts, {}), desc)
    return desc


def appear_boxes(frames, boxes, counts=None, out=None):
    """The appearance descriptors of boxes: a 128-bin colour histogram of 32 x 16 nearest-pixel samples over the central 0.75 of
    every box, in ONE launch (include/mydet.h: mydet_appear_boxes_rgb_u8, where the rule is).  frames: uint8 [B,H,W,3] or
    [H,W,3], read in place through their strides when pixels are packed.  boxes: float32 [B,K,4|5] or [K,4|5], K <= 512, rows (cx,
    cy, w, h[, degrees]) in frame pixels.  counts: int32 [B] (None: all K).  Returns uint16 [B,K,128]; every row is written, rows
    at or beyond the count are zeros.  out: such a tensor to write into (contiguous frames, any even frame stride)."""
    what = 'appear_boxes'
    return _appear_dense(what, *_image(what, frames, None, None, None, False), boxes, counts, out)


def appear_boxes_yuv420(planes, layout, boxes, counts=None, out=None, matrix='bt601', full_range=False):
    """appear_boxes out of 4:2:0 frames (mydet_appear_boxes_yuv420): the bits of appear_boxes on yuv420_to_rgb(planes, layout,
    matrix, full_range), which is never built.  Every layout, the 10-bit ones included."""
    what = 'appear_boxes_yuv420'
    return _appear_dense(what, *_image(what, planes, layout, matrix, full_range, False), boxes, counts, out)


def appear_records(source, rec, layout=None, out=None, matrix='bt601', full_range=False):
    """The descriptors of the detections of a record dict (ops.record_views; plain or rotated) in ONE launch that reads the
    record's planes in place -- nothing is copied or synchronised.  source: uint8 RGB frames [B,H,W,3] (layout None) or the
    planes of `layout`.  Returns uint16 [B,512,128], row = record slot: what track_frames takes as desc."""
    what = 'appear_records'
    records = _record_buffer(what, rec)
    image, yuv, B = _image(what, source, layout, matrix, full_range, False)
    if B != records.shape[0]:
        raise ValueError(f'{what}: {B} frames and {records.shape[0]} records')
    dev = _same_device(what, image, [records])
    desc = _appear_out(what, out, B, _lib.REC_TOPK, dev)
    _appear_launch(image, yuv, _list_of_records(what, records, False, None), desc)
    return desc


# --------------------------------------------------------------------------------------------------------------------------
# Scoring detections against ground truth (include/mydet.h: mydet_eval_set and the three mydet_eval_* launches; the rules are
# there).  eval_pack and eval_summarize are host numpy; everything between them runs on the device.
EVAL_KINDS = ('coco', 'cepdof')


class EvalParams:
    """The evaluation parameters of COCO's bbox evaluation, with its defaults: the attributes pycocotools' Params has."""

    def __init__(self):
        self.imgIds, self.catIds = [], []
        self.iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.areaRng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
        self.areaRngLbl = ['all', 'small', 'medium', 'large']
        self.useCats = 1
        self.useSegm = None
        self.iouType = 'bbox'


def _eval_kind(kind):
    if kind not in EVAL_KINDS:
        raise ValueError(f'kind {kind!r}: one of {EVAL_KINDS} expected')
    return kind == 'cepdof'


def eval_columns(rows, kind):
    """JSON detection rows -> the columns eval_pack takes: image_id and category_id (lists), bbox float64 [N, 4 | 5], score and
    area float64 [N].  area defaults to w*h; with kind 'cepdof' category_id defaults to 1."""
    width = 5 if _eval_kind(kind) else 4
    n = len(rows)
    return {'image_id': [r['image_id'] for r in rows],
            'category_id': [r.get('category_id', 1) for r in rows] if width == 5 else [r['category_id'] for r in rows],
            'bbox': np.array([r['bbox'][:width] for r in rows], dtype=np.float64).reshape(n, width),
            'score': np.array([r['score'] for r in rows], dtype=np.float64).reshape(n),
            'area': np.array([r['area'] if 'area' in r else r['bbox'][2] * r['bbox'][3] for r in rows], dtype=np.float64).reshape(n)}


def _eval_starts(groups, n):
    out = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(groups, minlength=n), out=out[1:])
    return out


def eval_pack(dts, gt, kind, max_det=100):
    """Host-only: detections (JSON rows, or the columns of eval_columns) and a loaded ground-truth dict ('images', 'categories',
    'annotations') -> the dense numpy arrays of mydet_eval_set (include/mydet.h, 'Packing'), cut to max_det = maxDets[-1] per
    group.  Beside the arrays the dict holds I, K, D, G, n_pairs, max_dt, max_gt, rotated, img_ids, cat_ids and dt_rows / gt_rows:
    the input row and the annotation each packed row came from."""
    rotated = _eval_kind(kind)
    width = 5 if rotated else 4
    cols = dts if isinstance(dts, dict) else eval_columns(dts, kind)
    img_ids = sorted(set(im['id'] for im in gt['images']))
    cat_ids = sorted(set(c['id'] for c in gt['categories']))
    I, K = len(img_ids), len(cat_ids)
    if I < 1 or K < 1 or I * K >= 2 ** 31:
        raise ValueError(f'eval_pack: {I} images x {K} categories')
    if int(max_det) < 1:
        raise ValueError(f'eval_pack: max_det {max_det}')
    img_index = {v: n for n, v in enumerate(img_ids)}
    cat_index = {v: n for n, v in enumerate(cat_ids)}

    def groups_of(images, cats):
        i = np.fromiter((img_index.get(v, -1) for v in images), dtype=np.int64, count=len(images))
        k = np.fromiter((cat_index.get(v, -1) for v in cats), dtype=np.int64, count=len(cats))
        keep = np.nonzero((i >= 0) & (k >= 0))[0]
        return keep, k[keep] * I + i[keep]

    anns = gt['annotations']
    keep, g = groups_of([a['image_id'] for a in anns], [a['category_id'] for a in anns])
    o = np.argsort(g, kind='stable')
    gt_rows, gt_g = keep[o], g[o]
    G = len(gt_rows)
    picked = [anns[r] for r in gt_rows]
    gt_box = np.array([a['bbox'][:width] for a in picked], dtype=np.float64).reshape(G, width)
    if rotated:
        gt_area = np.array([a['area'] if 'area' in a else a['bbox'][2] * a['bbox'][3] for a in picked], dtype=np.float64).reshape(G)
        ignore = [bool(a.get('ignore', False) or a.get('iscrowd', False)) for a in picked]
    else:
        gt_area = np.array([a['area'] for a in picked], dtype=np.float64).reshape(G)
        ignore = [bool(a.get('iscrowd', 0)) for a in picked]
    crowd = [bool(a.get('iscrowd', 0)) for a in picked]
    gt_flags = (np.array(ignore, dtype=np.uint8).reshape(G) * _lib.EVAL_GT_IGNORE
                + np.array(crowd, dtype=np.uint8).reshape(G) * _lib.EVAL_GT_CROWD).astype(np.uint8)
    gt_start = _eval_starts(gt_g, I * K)

    keep, g = groups_of(cols['image_id'], cols['category_id'])
    score = np.asarray(cols['score'], dtype=np.float64)[keep]
    o = np.lexsort((-score, g))                              # stable: equal scores of a group keep input order
    g = g[o]
    rank = np.arange(len(g), dtype=np.int64) - _eval_starts(g, I * K)[g]
    cut = rank < int(max_det)
    dt_rows, dt_g, dt_rank = keep[o][cut], g[cut], rank[cut]
    D = len(dt_rows)
    dt_box = np.asarray(cols['bbox'], dtype=np.float64).reshape(-1, width)[dt_rows]
    dt_score = np.asarray(cols['score'], dtype=np.float64)[dt_rows]
    dt_area = np.asarray(cols['area'], dtype=np.float64)[dt_rows]
    dt_start = _eval_starts(dt_g, I * K)
    dt_cat = dt_g // I
    order = np.lexsort((-dt_score, dt_cat))                  # stable: equal scores keep (image index, rank) order
    cat_start = _eval_starts(dt_cat, K)

    nd, ng = np.diff(dt_start), np.diff(gt_start)
    groups = np.nonzero((nd > 0) | (ng > 0))[0]
    pair_start = np.zeros(len(groups) + 1, dtype=np.int64)
    np.cumsum(nd[groups] * ng[groups], out=pair_start[1:])
    box_type = np.float32 if rotated else np.float64
    return {'kind': kind, 'rotated': int(rotated), 'I': I, 'K': K, 'D': D, 'G': G, 'n_pairs': int(pair_start[-1]),
            'max_dt': int(nd.max()) if D else 0, 'max_gt': int(ng.max()) if G else 0, 'img_ids': img_ids, 'cat_ids': cat_ids,
            'dt_rows': dt_rows, 'gt_rows': gt_rows,
            'groups': groups.astype(np.int32), 'pair_start': pair_start,
            'dt_start': dt_start.astype(np.int32), 'gt_start': gt_start.astype(np.int32),
            'dt_box': np.ascontiguousarray(dt_box.astype(box_type)), 'gt_box': np.ascontiguousarray(gt_box.astype(box_type)),
            'dt_score': dt_score, 'dt_area': dt_area, 'gt_area': gt_area, 'gt_flags': gt_flags,
            'dt_rank': dt_rank.astype(np.int32), 'order': order.astype(np.int32), 'cat_start': cat_start.astype(np.int32)}


EVAL_SET_ARRAYS = ('groups', 'dt_start', 'gt_start', 'pair_start', 'dt_box', 'gt_box', 'dt_score', 'dt_area', 'gt_area', 'gt_flags')


class EvalSet:
    """The arrays of eval_pack as tensors on one device (`.t`), with the mydet_eval_set that points at them (`.c`)."""

    def __init__(self, pack, device=None):
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError('EvalSet: no GPU is visible; mydetection_amd scores on MI355X only (there is no CPU path in this package)')
            device = 'cuda'
        self.pack = pack
        self.t = {k: torch.from_numpy(np.ascontiguousarray(pack[k])).to(device) for k in EVAL_SET_ARRAYS + ('dt_rank', 'order', 'cat_start')}
        require_gpu(self.t['dt_start'], 'EvalSet')
        self.device = self.t['dt_start'].device
        self.c = eval_set_struct(pack, {k: self.t[k].data_ptr() for k in EVAL_SET_ARRAYS})


def eval_set_struct(pack, pointers):
    """_lib.EvalSet from the scalars of a pack and a name -> address mapping (a null pointer for an absent or empty array)."""
    c = _lib.EvalSet()
    for k in ('rotated', 'I', 'K', 'max_dt', 'max_gt', 'D', 'G', 'n_pairs'):
        setattr(c, k, int(pack[k]))
    c.n_groups = len(pack['groups'])
    for k in EVAL_SET_ARRAYS:
        setattr(c, k, pointers.get(k) if len(pack[k]) else None)
    return c


def _eval_thresholds(values, what, width=None):
    a = np.ascontiguousarray(np.asarray(values, dtype=np.float64))
    if width is not None:
        a = np.ascontiguousarray(a.reshape(-1, width))
    elif a.ndim != 1:
        raise ValueError(f'{what}: a 1-d array expected')
    return a


def eval_ious(es):
    """float64 [n_pairs]: the IoU of every (detection, ground truth) pair of every group, one launch."""
    out = torch.empty((es.pack['n_pairs'],), dtype=torch.float64, device=es.device)
    with torch.cuda.device(es.device):
        code = _lib.lib().mydet_eval_ious_f64(ctypes.byref(es.c), _ptr(out), _stream())
    _lib.check(code, 'mydet_eval_ious_f64')
    return out


def eval_match(es, ious, iou_thrs, area_rng, rows=False):
    """The greedy matching of every group at every (area range, IoU threshold), one launch: (matched, ignored, gt_row).  matched
    and ignored are int32 [A, D] holding 32-bit masks over the thresholds (bit t); gt_row is int32 [A, T, D], the matched
    ground-truth row or -1 (None unless rows=True)."""
    thr, rng = _eval_thresholds(iou_thrs, 'iou_thrs'), _eval_thresholds(area_rng, 'area_rng', 2)
    D, T, A = es.pack['D'], len(thr), len(rng)
    require_gpu(ious, 'eval_match')
    if ious.dtype != torch.float64 or ious.numel() != es.pack['n_pairs'] or not ious.is_contiguous():
        raise ValueError(f"eval_match: ious must be float64 [{es.pack['n_pairs']}], contiguous")
    matched = torch.empty((A, D), dtype=torch.int32, device=es.device)         # the launch writes every row: each detection
    ignored = torch.empty((A, D), dtype=torch.int32, device=es.device)         # belongs to a listed group
    gt_row = torch.empty((A, T, D), dtype=torch.int32, device=es.device) if rows else None
    with torch.cuda.device(es.device):
        code = _lib.lib().mydet_eval_match_f64(ctypes.byref(es.c), _ptr(ious), thr.ctypes.data, T, rng.ctypes.data, A, _ptr(matched),
                                               _ptr(ignored), _ptr(gt_row), _stream())
    _lib.check(code, 'mydet_eval_match_f64')
    return matched, ignored, gt_row


def eval_accumulate(es, matched, ignored, n_thrs, area_rng, max_dets, rec_thrs):
    """precision [T,R,K,A,M], recall [T,K,A,M], scores [T,R,K,A,M] (float64 tensors) from the masks of eval_match, one launch."""
    rng, rec = _eval_thresholds(area_rng, 'area_rng', 2), _eval_thresholds(rec_thrs, 'rec_thrs')
    md = np.ascontiguousarray(np.asarray(max_dets, dtype=np.int32))
    T, A, M, R, K, D = int(n_thrs), len(rng), len(md), len(rec), es.pack['K'], es.pack['D']
    for name, m in (('matched', matched), ('ignored', ignored)):
        require_gpu(m, 'eval_accumulate')
        if m.dtype != torch.int32 or tuple(m.shape) != (A, D) or not m.is_contiguous():
            raise ValueError(f'eval_accumulate: {name} must be int32 [{A}, {D}], contiguous')
    precision = torch.empty((T, R, K, A, M), dtype=torch.float64, device=es.device)
    recall = torch.empty((T, K, A, M), dtype=torch.float64, device=es.device)
    scores = torch.empty((T, R, K, A, M), dtype=torch.float64, device=es.device)
    t = es.t
    with torch.cuda.device(es.device):
        code = _lib.lib().mydet_eval_accumulate_f64(ctypes.byref(es.c), _ptr(t['order']), _ptr(t['cat_start']), _ptr(t['dt_rank']),
                                                    _ptr(matched), _ptr(ignored), T, rng.ctypes.data, A, md.ctypes.data, M, rec.ctypes.data,
                                                    R, _ptr(precision), _ptr(recall), _ptr(scores), _stream())
    _lib.check(code, 'mydet_eval_accumulate_f64')
    return precision, recall, scores


EVAL_SUMMARY_ROW = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'


def eval_summarize(precision, recall, params):
    """Host numpy: the 12 stats and the summary text of COCO's bbox evaluation from precision [T,R,K,A,M] and recall [T,K,A,M]
    (numpy arrays) -- the reference's summarize(), its row format and selection rules: the mean over the entries > -1 of the
    selected threshold, area label and maxDets, and -1 when there are none.  Like the reference it needs params.maxDets[2]."""
    precision, recall = np.asarray(precision), np.asarray(recall)
    iou_thrs = np.asarray(params.iouThrs)
    lines = []

    def row(ap, iou=None, area='all', max_dets=100):
        a_sel = [n for n, lbl in enumerate(params.areaRngLbl) if lbl == area]
        m_sel = [n for n, v in enumerate(params.maxDets) if v == max_dets]
        s = precision if ap else recall
        if iou is not None:
            s = s[np.where(iou == iou_thrs)[0]]
        s = s[..., a_sel, m_sel]
        found = s[s > -1]
        mean = -1 if len(found) == 0 else np.mean(found)
        span = '{:0.2f}:{:0.2f}'.format(iou_thrs[0], iou_thrs[-1]) if iou is None else '{:0.2f}'.format(iou)
        lines.append(EVAL_SUMMARY_ROW.format('Average Precision' if ap else 'Average Recall', '(AP)' if ap else '(AR)', span, area,
                                             max_dets, mean))
        return mean

    top = params.maxDets[2]
    stats = np.zeros((12,))
    stats[0] = row(1)
    stats[1] = row(1, iou=.5, max_dets=top)
    stats[2] = row(1, iou=.75, max_dets=top)
    for n, area in enumerate(('small', 'medium', 'large')):
        stats[3 + n] = row(1, area=area, max_dets=top)
    for n in range(3):
        stats[6 + n] = row(0, max_dets=params.maxDets[n])
    for n, area in enumerate(('small', 'medium', 'large')):
        stats[9 + n] = row(0, area=area, max_dets=top)
    return stats, ''.join(line + '\n' for line in lines)


# --------------------------------------------------------------------------------------------------------------------------
# Scoring tracks against ground truth (include/mydet.h: mydet_mot_set and the three mydet_mot_* launches; the rules are there).
# mot_pack and mot_summarize are host numpy; everything between them runs on the device.
MOT_ID_KEYS = ('track_id', 'person_id')
MOT_COUNTS = ('tp', 'fp', 'fn', 'idsw', 'frag')


def mot_columns(rows, kind):
    """JSON hypothesis rows that carry 'track_id' -> the columns mot_pack takes: image_id, category_id and track_id (lists),
    bbox float64 [N, 4 | 5].  With kind 'cepdof' category_id defaults to 1."""
    width = 5 if _eval_kind(kind) else 4
    for r in rows:
        if 'track_id' not in r:
            raise ValueError("mot_columns: a hypothesis row without 'track_id'")
        if len(r['bbox']) < width:
            raise ValueError(f"mot_columns: kind {kind!r} scores {width}-wide boxes, got {len(r['bbox'])}")
    return {'image_id': [r['image_id'] for r in rows],
            'category_id': [r.get('category_id', 1) for r in rows] if width == 5 else [r['category_id'] for r in rows],
            'track_id': [r['track_id'] for r in rows],
            'bbox': np.array([r['bbox'][:width] for r in rows], dtype=np.float64).reshape(len(rows), width)}


def mot_sequences(gt, sequences=None):
    """(names, [image ids of each sequence in frame order]).  sequences: a dict {name: [img_id, ...]} gives them explicitly; None
    groups the images by 'video_id' ordered by 'frame_id' when every image has both, and otherwise makes one sequence in
    `images` order."""
    images = gt['images']
    if sequences is not None:
        names = list(sequences)
        frames = [list(sequences[n]) for n in names]
        known = set(im['id'] for im in images)
        for n, ids in zip(names, frames):
            missing = [i for i in ids if i not in known]
            if missing:
                raise ValueError(f'sequence {n!r}: image id {missing[0]!r} is not in the ground truth')
    elif images and all('video_id' in im and 'frame_id' in im for im in images):
        by = {}
        for im in images:
            by.setdefault(im['video_id'], []).append((im['frame_id'], im['id']))
        names = sorted(by)
        frames = [[i for _, i in sorted(by[n])] for n in names]
    else:
        names, frames = ['all'], [[im['id'] for im in images]]
    flat = [i for ids in frames for i in ids]
    if len(set(flat)) != len(flat):
        raise ValueError('mot_sequences: an image id appears in more than one frame')
    if not flat:
        raise ValueError('mot_sequences: no frames')
    return names, frames


def mot_id_key(gt, id_key=None):
    """The identity key of the ground-truth annotations: id_key, or the first of 'track_id' and 'person_id' they carry."""
    anns = gt['annotations']
    keys = (id_key,) if id_key is not None else MOT_ID_KEYS
    for key in keys:
        if all(key in a for a in anns):
            return key
    raise ValueError(f'ground-truth annotations without an identity: one of {keys} expected in every annotation')


def _mot_side(images, cats, ids, frame_of, cat_of, seq_of, I, S, what):
    """The packed order of one side (stable by group), its groups, and its dense identities per unit."""
    f = np.fromiter((frame_of.get(v, -1) for v in images), dtype=np.int64, count=len(images))
    k = np.fromiter((cat_of(v) for v in cats), dtype=np.int64, count=len(cats))
    keep = np.nonzero((f >= 0) & (k >= 0))[0]
    g = k[keep] * I + f[keep]
    o = np.argsort(g, kind='stable')
    rows, g = keep[o], g[o]
    unit = (g // I) * S + seq_of[g % I]
    dense = np.zeros(len(rows), dtype=np.int32)
    tables, seen = {}, set()
    for n, (r, gg, u) in enumerate(zip(rows.tolist(), g.tolist(), unit.tolist())):
        table = tables.setdefault(u, {})
        dense[n] = table.setdefault(ids[r], len(table))
        if (gg, dense[n]) in seen:
            raise ValueError(f'mot_pack: {what} identity {ids[r]!r} appears twice in image {images[r]!r}')
        seen.add((gg, dense[n]))
    return rows, g, dense, tables


def mot_pack(dts, gt, kind, sequences=None, id_key=None, use_cats=True):
    """Host-only: hypotheses (JSON rows with 'track_id', or the columns of mot_columns) and a loaded ground-truth dict -> the dense
    numpy arrays of mydet_eval_set and mydet_mot_set (include/mydet.h, 'Data model').  Frames are the images of the sequences laid
    end to end (mot_sequences); categories are the sorted category ids, or one category with use_cats=False; rows keep input order
    inside their group.  Beside the arrays the dict holds the scalars, seq_names, cat_ids, img_ids (frame order), dt_rows / gt_rows
    and gt_ids / dt_ids: per unit, the identity of every dense index.  A duplicate identity in a frame is a ValueError."""
    rotated = _eval_kind(kind)
    width = 5 if rotated else 4
    cols = dts if isinstance(dts, dict) else mot_columns(dts, kind)
    names, frames = mot_sequences(gt, sequences)
    img_ids = [i for ids in frames for i in ids]
    cat_ids = sorted(set(c['id'] for c in gt['categories'])) if use_cats else [None]
    I, S, K = len(img_ids), len(names), len(cat_ids)
    if K < 1 or I * K >= 2 ** 31:
        raise ValueError(f'mot_pack: {I} frames x {K} categories')
    U = S * K
    seq_start = np.zeros(S + 1, dtype=np.int64)
    np.cumsum([len(ids) for ids in frames], out=seq_start[1:])
    seq_of = np.repeat(np.arange(S), np.diff(seq_start))
    frame_of = {v: n for n, v in enumerate(img_ids)}
    cat_index = {v: n for n, v in enumerate(cat_ids)}
    cat_of = (lambda v: cat_index.get(v, -1)) if use_cats else (lambda v: 0)

    anns = gt['annotations']
    key = mot_id_key(gt, id_key)
    for a in anns:
        if len(a['bbox']) < width:
            raise ValueError(f"mot_pack: kind {kind!r} scores {width}-wide boxes, got {len(a['bbox'])} in the ground truth")
    gt_rows, gt_g, gt_id, gt_tables = _mot_side([a['image_id'] for a in anns], [a.get('category_id', 1) for a in anns],
                                                [a[key] for a in anns], frame_of, cat_of, seq_of, I, S, 'ground-truth')
    dt_box_in = np.asarray(cols['bbox'], dtype=np.float64)
    if dt_box_in.size and (dt_box_in.ndim != 2 or dt_box_in.shape[1] != width):
        raise ValueError(f'mot_pack: kind {kind!r} scores {width}-wide boxes, got {dt_box_in.shape}')
    dt_rows, dt_g, dt_id, dt_tables = _mot_side(cols['image_id'], cols['category_id'], cols['track_id'], frame_of, cat_of, seq_of,
                                                I, S, 'hypothesis')
    G, D = len(gt_rows), len(dt_rows)
    gt_box = np.array([anns[r]['bbox'][:width] for r in gt_rows], dtype=np.float64).reshape(G, width)
    dt_box = dt_box_in.reshape(-1, width)[dt_rows]
    gt_start, dt_start = _eval_starts(gt_g, I * K), _eval_starts(dt_g, I * K)
    nd, ng = np.diff(dt_start), np.diff(gt_start)
    groups = np.nonzero((nd > 0) | (ng > 0))[0]
    pair_start = np.zeros(len(groups) + 1, dtype=np.int64)
    np.cumsum(nd[groups] * ng[groups], out=pair_start[1:])
    n_gid = np.array([len(gt_tables.get(u, ())) for u in range(U)], dtype=np.int64)
    n_hid = np.array([len(dt_tables.get(u, ())) for u in range(U)], dtype=np.int64)
    gt_id_start, dt_id_start, ov_start = (np.zeros(U + 1, dtype=np.int64) for _ in range(3))
    np.cumsum(n_gid, out=gt_id_start[1:])
    np.cumsum(n_hid, out=dt_id_start[1:])
    np.cumsum(n_gid * n_hid, out=ov_start[1:])
    if gt_id_start[-1] >= 2 ** 31 or dt_id_start[-1] >= 2 ** 31:
        raise ValueError('mot_pack: too many identities')
    box_type = np.float32 if rotated else np.float64
    return {'kind': kind, 'rotated': int(rotated), 'I': I, 'K': K, 'S': S, 'U': U, 'D': D, 'G': G, 'n_pairs': int(pair_start[-1]),
            'max_dt': int(nd.max()) if D else 0, 'max_gt': int(ng.max()) if G else 0,
            'max_gt_ids': int(n_gid.max()), 'max_dt_ids': int(n_hid.max()), 'n_gt_ids': int(gt_id_start[-1]),
            'n_dt_ids': int(dt_id_start[-1]), 'n_ov': int(ov_start[-1]),
            'img_ids': img_ids, 'cat_ids': cat_ids, 'seq_names': names, 'dt_rows': dt_rows, 'gt_rows': gt_rows,
            'gt_ids': [list(gt_tables.get(u, ())) for u in range(U)], 'dt_ids': [list(dt_tables.get(u, ())) for u in range(U)],
            'groups': groups.astype(np.int32), 'pair_start': pair_start,
            'dt_start': dt_start.astype(np.int32), 'gt_start': gt_start.astype(np.int32),
            'dt_box': np.ascontiguousarray(dt_box.astype(box_type)), 'gt_box': np.ascontiguousarray(gt_box.astype(box_type)),
            'dt_score': np.ones(D), 'dt_area': dt_box[:, 2] * dt_box[:, 3], 'gt_area': gt_box[:, 2] * gt_box[:, 3],
            'gt_flags': np.zeros(G, dtype=np.uint8),
            'seq_start': seq_start.astype(np.int32), 'gt_id': gt_id, 'dt_id': dt_id,
            'gt_id_start': gt_id_start.astype(np.int32), 'dt_id_start': dt_id_start.astype(np.int32), 'ov_start': ov_start}


MOT_SET_ARRAYS = ('seq_start', 'gt_id', 'dt_id', 'gt_id_start', 'dt_id_start', 'ov_start')


def mot_set_struct(pack, pointers):
    """_lib.MotSet from the scalars of a pack and a name -> address mapping (a null pointer for an absent or empty array)."""
    c = _lib.MotSet()
    for k in ('S', 'max_gt_ids', 'max_dt_ids', 'n_gt_ids', 'n_dt_ids', 'n_ov'):
        setattr(c, k, int(pack[k]))
    for k in MOT_SET_ARRAYS:
        setattr(c, k, pointers.get(k) if len(pack[k]) else None)
    return c


class MotSet:
    """The arrays of mot_pack as tensors on one device (`.t`), with the mydet_eval_set (`.c`) and the mydet_mot_set (`.m`) that
    point at them."""

    def __init__(self, pack, device=None):
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError('MotSet: no GPU is visible; mydetection_amd scores on MI355X only (there is no CPU path in this package)')
            device = 'cuda'
        self.pack = pack
        self.t = {k: torch.from_numpy(np.ascontiguousarray(pack[k])).to(device) for k in EVAL_SET_ARRAYS + MOT_SET_ARRAYS}
        require_gpu(self.t['dt_start'], 'MotSet')
        self.device = self.t['dt_start'].device
        self.c = eval_set_struct(pack, {k: self.t[k].data_ptr() for k in EVAL_SET_ARRAYS})
        self.m = mot_set_struct(pack, {k: self.t[k].data_ptr() for k in MOT_SET_ARRAYS})


def mot_clear(ms, ious, iou_thrs, rows=False):
    """mydet_mot_clear_f64, one launch: (counts int64 [U, T, 5] = (TP, FP, FN, IDSW, FRAG), siou float64 [U, T], present int32
    [Gids], matched int32 [T, Gids], gt_match int32 [T, G] or None unless rows=True)."""
    thr = _eval_thresholds(iou_thrs, 'iou_thrs')
    p, T, dev = ms.pack, len(thr), ms.device
    counts = torch.empty((p['U'], T, 5), dtype=torch.int64, device=dev)
    siou = torch.empty((p['U'], T), dtype=torch.float64, device=dev)
    present = torch.empty((p['n_gt_ids'],), dtype=torch.int32, device=dev)
    matched = torch.empty((T, p['n_gt_ids']), dtype=torch.int32, device=dev)
    gt_match = torch.empty((T, p['G']), dtype=torch.int32, device=dev) if rows else None
    with torch.cuda.device(dev):
        code = _lib.lib().mydet_mot_clear_f64(ctypes.byref(ms.c), ctypes.byref(ms.m), _ptr(ious), thr.ctypes.data, T, _ptr(counts),
                                              _ptr(siou), _ptr(present), _ptr(matched), _ptr(gt_match), _stream())
    _lib.check(code, 'mydet_mot_clear_f64')
    return counts, siou, present, matched, gt_match


def mot_id_overlap(ms, ious, iou_thrs):
    """mydet_mot_id_overlap (a memset and one launch): int32 [T, n_ov], per threshold the identity-overlap matrix of every unit,
    unit u's [nG_u, nH_u] block at ov_start[u].  The tensor is the scratch mydet_mot_scratch_bytes sizes."""
    thr = _eval_thresholds(iou_thrs, 'iou_thrs')
    T = len(thr)
    overlap = torch.empty((T, ms.pack['n_ov']), dtype=torch.int32, device=ms.device)
    with torch.cuda.device(ms.device):
        nbytes = _lib.lib().mydet_mot_scratch_bytes(ctypes.byref(ms.m), T)
        if T <= _lib.EVAL_MAX_THRS and nbytes != overlap.numel() * 4:
            raise RuntimeError(f'mydet_mot_scratch_bytes: {nbytes} for [{T}, {ms.pack["n_ov"]}] int32')
        code = _lib.lib().mydet_mot_id_overlap(ctypes.byref(ms.c), ctypes.byref(ms.m), _ptr(ious), thr.ctypes.data, T, _ptr(overlap),
                                               nbytes, _stream())
    _lib.check(code, 'mydet_mot_id_overlap')
    return overlap


def mot_id_assign(ms, overlap):
    """mydet_mot_id_assign, one launch: IDTP int64 [U, T] from the matrices of mot_id_overlap."""
    T = overlap.shape[0]
    require_gpu(overlap, 'mot_id_assign')
    if overlap.dtype != torch.int32 or tuple(overlap.shape) != (T, ms.pack['n_ov']) or not overlap.is_contiguous():
        raise ValueError(f"mot_id_assign: overlap must be int32 [T, {ms.pack['n_ov']}], contiguous")
    idtp = torch.empty((ms.pack['U'], T), dtype=torch.int64, device=ms.device)
    with torch.cuda.device(ms.device):
        code = _lib.lib().mydet_mot_id_assign(ctypes.byref(ms.c), ctypes.byref(ms.m), T, _ptr(overlap), overlap.numel() * 4, _ptr(idtp),
                                              _stream())
    _lib.check(code, 'mydet_mot_id_assign')
    return idtp


def mot_evaluate(ms, iou_thrs, rows=False, ious=None):
    """The four launches on a MotSet (or a pack): mydet_eval_ious_f64, mydet_mot_clear_f64, mydet_mot_id_overlap and
    mydet_mot_id_assign, stream-ordered, no synchronisation.  Returns the raw arrays as tensors: counts, siou, present, matched and
    gt_match (mot_clear), idtp int64 [U, T], ious float64 [n_pairs] and overlap int32 [T, n_ov].  ious: a float64 [n_pairs] tensor
    to score instead of the IoUs of the boxes."""
    if isinstance(ms, dict):
        ms = MotSet(ms)
    if ious is None:
        ious = eval_ious(ms)
    else:
        require_gpu(ious, 'mot_evaluate')
        if ious.dtype != torch.float64 or ious.numel() != ms.pack['n_pairs'] or not ious.is_contiguous() or ious.device != ms.device:
            raise ValueError(f"mot_evaluate: ious must be float64 [{ms.pack['n_pairs']}], contiguous, on {ms.device}")
    counts, siou, present, matched, gt_match = mot_clear(ms, ious, iou_thrs, rows)
    overlap = mot_id_overlap(ms, ious, iou_thrs)
    idtp = mot_id_assign(ms, overlap)
    return {'counts': counts, 'siou': siou, 'present': present, 'matched': matched, 'idtp': idtp, 'ious': ious, 'overlap': overlap,
            'gt_match': gt_match}


def _mot_ratio(num, den):
    """One float64 division of two exact integers; nan without a denominator."""
    return float(np.float64(num) / np.float64(den)) if den else float('nan')


def mot_metrics(tp, fp, fn, idsw, frag, siou, idtp, present, matched):
    """Host: the metrics of one row (a sequence or the total) at one threshold from its integer counts, SIOU and the present /
    matched frame counts of its ground-truth identities.  motp is the mean IoU of the matches, not a distance.  Mostly tracked is
    5 * matched >= 4 * present, mostly lost 5 * matched < present, both in integers."""
    tp, fp, fn, idsw, frag, idtp = (int(v) for v in (tp, fp, fn, idsw, frag, idtp))
    n_gt, n_hyp = tp + fn, tp + fp
    present, matched = np.asarray(present, dtype=np.int64), np.asarray(matched, dtype=np.int64)
    mt = int(np.count_nonzero(5 * matched >= 4 * present))
    ml = int(np.count_nonzero(5 * matched < present))
    mota = _mot_ratio(fn + fp + idsw, n_gt)
    return {'tp': tp, 'fp': fp, 'fn': fn, 'idsw': idsw, 'frag': frag, 'n_gt': n_gt, 'n_hyp': n_hyp,
            'idtp': idtp, 'idfp': n_hyp - idtp, 'idfn': n_gt - idtp,
            'mota': 1.0 - mota, 'motp': _mot_ratio(siou, tp) if tp else float('nan'),
            'precision': _mot_ratio(tp, n_hyp), 'recall': _mot_ratio(tp, n_gt),
            'idf1': _mot_ratio(2 * idtp, n_gt + n_hyp), 'idp': _mot_ratio(idtp, n_hyp), 'idr': _mot_ratio(idtp, n_gt),
            'n_ids': int(len(present)), 'mt': mt, 'pt': int(len(present)) - mt - ml, 'ml': ml}


MOT_SUMMARY_COLUMNS = ('mota', 'motp', 'idf1', 'idp', 'idr', 'recall', 'precision')
MOT_SUMMARY_COUNTS = ('n_ids', 'mt', 'pt', 'ml', 'tp', 'fp', 'fn', 'idsw', 'frag')


def mot_summarize(raw, pack, iou_thrs):
    """Host numpy: per sequence and overall, per threshold, the metrics of mot_metrics from the raw arrays of mot_evaluate (numpy).
    A sequence sums its categories' units; SIOU is added unit by unit in unit order.  Returns (result, text): result is
    {'iou_thrs', 'overall': [per threshold], 'sequences': {name: [per threshold]}}."""
    S, K, T = pack['S'], pack['K'], len(iou_thrs)
    counts, siou, idtp = np.asarray(raw['counts']), np.asarray(raw['siou']), np.asarray(raw['idtp'])
    present, matched = np.asarray(raw['present']), np.asarray(raw['matched'])
    ids = pack['gt_id_start']

    def row(units, t):
        c = sum((counts[u, t].astype(np.int64) for u in units), np.zeros(5, dtype=np.int64))
        s = np.float64(0.0)
        for u in units:
            s = s + siou[u, t]
        sel = np.concatenate([np.arange(ids[u], ids[u + 1]) for u in units]) if units else np.zeros(0, dtype=np.int64)
        return mot_metrics(c[0], c[1], c[2], c[3], c[4], s, sum(int(idtp[u, t]) for u in units), present[sel], matched[t][sel])

    result = {'iou_thrs': [float(v) for v in iou_thrs],
              'sequences': {name: [row([k * S + s for k in range(K)], t) for t in range(T)] for s, name in enumerate(pack['seq_names'])},
              'overall': [row(list(range(S * K)), t) for t in range(T)]}
    head = ' {:<16} {:>5}'.format('sequence', 'IoU') + ''.join(' {:>9}'.format(c) for c in MOT_SUMMARY_COLUMNS) \
        + ''.join(' {:>6}'.format(c) for c in MOT_SUMMARY_COUNTS)
    lines = [head]
    for name, rows in list(result['sequences'].items()) + [('OVERALL', result['overall'])]:
        for t, r in enumerate(rows):
            lines.append(' {:<16} {:>5.2f}'.format(str(name)[:16], result['iou_thrs'][t]) + ''.join(' {:>9.4f}'.format(r[c]) for c in MOT_SUMMARY_COLUMNS)
                         + ''.join(' {:>6d}'.format(r[c]) for c in MOT_SUMMARY_COUNTS))
    return result, ''.join(line + '\n' for line in lines)


# --------------------------------------------------------------------------------------------------------------------------
# HOTA on the same packed arrays (include/mydet.h, "HOTA": the three mydet_hota_* launches; the rules are there).  Everything up to
# hota_summarize runs on the device; hota_summarize is host numpy.
HOTA_DEFAULT_ALPHAS = tuple((np.arange(1, 20) / 20.0).tolist())
HOTA_COUNTS = ('tp', 'fn', 'fp')
HOTA_PER_ALPHA = ('hota', 'deta', 'assa', 'detre', 'detpr', 'assre', 'asspr', 'loca')


def hota_alphas(alphas=True):
    """The float64 array of localisation thresholds: True (or None) gives 0.05 .. 0.95; a sequence gives its values, 1 to
    EVAL_MAX_THRS of them, each > 0, <= 1 and not NaN (ValueError otherwise)."""
    a = np.array(HOTA_DEFAULT_ALPHAS) if alphas is True or alphas is None else _eval_thresholds(alphas, 'alphas')
    if not 1 <= len(a) <= _lib.EVAL_MAX_THRS:
        raise ValueError(f'hota: 1 to {_lib.EVAL_MAX_THRS} alphas expected, got {len(a)}')
    if not bool(np.all((a > 0) & (a <= 1))):                         # NaN fails both
        raise ValueError('hota: every alpha must be > 0 and <= 1, none of them NaN')
    return a


def _hota_tensor(what, t, dtype, n, dev, name):
    require_gpu(t, what)
    if t.dtype != dtype or t.numel() != n or not t.is_contiguous() or t.device != dev:
        raise ValueError(f'{what}: {name} must be {dtype} with {n} elements, contiguous, on {dev}')
    return t


def hota_align(ms, ious):
    """mydet_hota_align_f64 (three memsets and two launches): (pot int64 [n_ov], gt_count int32 [Gids], dt_count int32 [Hids]):
    the fixed-point alignment potentials of every identity pair, unit u's [nG_u, nH_u] block at ov_start[u], and the number of
    frames every identity is present in."""
    p, dev = ms.pack, ms.device
    _hota_tensor('hota_align', ious, torch.float64, p['n_pairs'], dev, 'ious')
    pot = torch.empty((p['n_ov'],), dtype=torch.int64, device=dev)
    gt_count = torch.empty((p['n_gt_ids'],), dtype=torch.int32, device=dev)
    dt_count = torch.empty((p['n_dt_ids'],), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        code = _lib.lib().mydet_hota_align_f64(ctypes.byref(ms.c), ctypes.byref(ms.m), _ptr(ious), _ptr(pot), _ptr(gt_count),
                                               _ptr(dt_count), _stream())
    _lib.check(code, 'mydet_hota_align_f64')
    return pot, gt_count, dt_count


def hota_match(ms, ious, pot, gt_count, dt_count):
    """mydet_hota_match (two memsets and one launch, one wavefront per listed group): (score_q int32 [n_pairs], the pair scores in
    the layout of ious; hota_match int32 [G], the assigned hypothesis row of every ground truth or -1).  Independent of alpha."""
    p, dev = ms.pack, ms.device
    _hota_tensor('hota_match', ious, torch.float64, p['n_pairs'], dev, 'ious')
    _hota_tensor('hota_match', pot, torch.int64, p['n_ov'], dev, 'pot')
    _hota_tensor('hota_match', gt_count, torch.int32, p['n_gt_ids'], dev, 'gt_count')
    _hota_tensor('hota_match', dt_count, torch.int32, p['n_dt_ids'], dev, 'dt_count')
    score_q = torch.empty((p['n_pairs'],), dtype=torch.int32, device=dev)
    match = torch.empty((p['G'],), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        code = _lib.lib().mydet_hota_match(ctypes.byref(ms.c), ctypes.byref(ms.m), _ptr(ious), _ptr(pot), _ptr(gt_count), _ptr(dt_count),
                                           _ptr(score_q), _ptr(match), _stream())
    _lib.check(code, 'mydet_hota_match')
    return score_q, match


def hota_score(ms, ious, match, gt_count, dt_count, alphas):
    """mydet_hota_score_f64 (a memset and two launches): (counts int64 [U, T, 3] = (TP, FN, FP), matches int32 [T, n_ov], loc_sum
    float64 [U, T], ass_sum float64 [U, T, 3])."""
    a = hota_alphas(alphas)
    p, T, dev = ms.pack, len(a), ms.device
    _hota_tensor('hota_score', ious, torch.float64, p['n_pairs'], dev, 'ious')
    _hota_tensor('hota_score', match, torch.int32, p['G'], dev, 'hota_match')
    _hota_tensor('hota_score', gt_count, torch.int32, p['n_gt_ids'], dev, 'gt_count')
    _hota_tensor('hota_score', dt_count, torch.int32, p['n_dt_ids'], dev, 'dt_count')
    counts = torch.empty((p['U'], T, 3), dtype=torch.int64, device=dev)
    matches = torch.empty((T, p['n_ov']), dtype=torch.int32, device=dev)
    loc_sum = torch.empty((p['U'], T), dtype=torch.float64, device=dev)
    ass_sum = torch.empty((p['U'], T, 3), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        code = _lib.lib().mydet_hota_score_f64(ctypes.byref(ms.c), ctypes.byref(ms.m), _ptr(ious), _ptr(match), _ptr(gt_count),
                                               _ptr(dt_count), a.ctypes.data, T, _ptr(counts), _ptr(matches), _ptr(loc_sum),
                                               _ptr(ass_sum), _stream())
    _lib.check(code, 'mydet_hota_score_f64')
    return counts, matches, loc_sum, ass_sum


def hota_evaluate(ms, alphas=True, ious=None):
    """mydet_eval_ious_f64 and the three HOTA launches on a MotSet (or a pack), stream-ordered, no synchronisation.  Returns the
    raw arrays as tensors: ious, pot, gt_count, dt_count, score_q, hota_match, counts, matches, loc_sum, ass_sum.  ious: a float64
    [n_pairs] tensor to score instead of the IoUs of the boxes (mot_evaluate's, for one)."""
    a = hota_alphas(alphas)
    if isinstance(ms, dict):
        ms = MotSet(ms)
    if ious is None:
        ious = eval_ious(ms)
    pot, gt_count, dt_count = hota_align(ms, ious)
    score_q, match = hota_match(ms, ious, pot, gt_count, dt_count)
    counts, matches, loc_sum, ass_sum = hota_score(ms, ious, match, gt_count, dt_count, a)
    return {'ious': ious, 'pot': pot, 'gt_count': gt_count, 'dt_count': dt_count, 'score_q': score_q, 'hota_match': match,
            'counts': counts, 'matches': matches, 'loc_sum': loc_sum, 'ass_sum': ass_sum}


def _hota_ratio(num, den):
    """One float64 division; 0.0 without a denominator."""
    return float(np.float64(num) / np.float64(den)) if den else 0.0


def hota_metrics(tp, fn, fp, loc_sum, ass_sum):
    """Host: the metrics of one row (a sequence or the total) at one alpha from its integer counts and the two float64 sums."""
    tp, fn, fp = int(tp), int(fn), int(fp)
    deta = _hota_ratio(tp, tp + fn + fp)
    assa, assre, asspr = (_hota_ratio(v, max(1, tp)) for v in ass_sum)
    return {'tp': tp, 'fn': fn, 'fp': fp, 'deta': deta, 'detre': _hota_ratio(tp, tp + fn), 'detpr': _hota_ratio(tp, tp + fp),
            'assa': assa, 'assre': assre, 'asspr': asspr, 'loca': _hota_ratio(loc_sum, tp) if tp else 1.0,
            'hota': float(np.sqrt(np.float64(deta) * np.float64(assa)))}


HOTA_SUMMARY_COLUMNS = ('hota', 'deta', 'assa', 'detre', 'detpr', 'assre', 'asspr', 'loca', 'hota0', 'loca0', 'hota_loca0')


def hota_summarize(raw, pack, alphas):
    """Host numpy: per sequence and overall, the HOTA family from the raw arrays of hota_evaluate (numpy).  A sequence row sums its
    categories' units and the overall row sums all units, as the CLEAR rows do (not TrackEval's averaging over classes); the float64
    sums are added unit by unit in unit order.  Returns (result, text): result is {'alphas', 'overall': entry, 'sequences':
    {name: entry}}; an entry holds 'per_alpha', the lists tp, fn, fp, hota, deta, assa, detre, detpr, assre, asspr and loca over
    the alphas, and as scalars under the same names the means of the ratios over the alphas, plus hota0, loca0 and hota_loca0 =
    hota0 * loca0 at the first alpha."""
    S, K, T = pack['S'], pack['K'], len(alphas)
    counts, loc_sum, ass_sum = np.asarray(raw['counts']), np.asarray(raw['loc_sum']), np.asarray(raw['ass_sum'])

    def entry(units):
        rows = []
        for t in range(T):
            c = sum((counts[u, t].astype(np.int64) for u in units), np.zeros(3, dtype=np.int64))
            loc, ass = np.float64(0.0), np.zeros(3, dtype=np.float64)
            for u in units:
                loc = loc + loc_sum[u, t]
                ass = ass + ass_sum[u, t]
            rows.append(hota_metrics(c[0], c[1], c[2], loc, ass))
        out = {'per_alpha': {k: [r[k] for r in rows] for k in HOTA_COUNTS + HOTA_PER_ALPHA}}
        for k in HOTA_PER_ALPHA:
            out[k] = float(np.mean(np.array(out['per_alpha'][k], dtype=np.float64)))
        out['hota0'], out['loca0'] = rows[0]['hota'], rows[0]['loca']
        out['hota_loca0'] = float(np.float64(out['hota0']) * np.float64(out['loca0']))
        return out

    result = {'alphas': [float(v) for v in alphas],
              'sequences': {name: entry([k * S + s for k in range(K)]) for s, name in enumerate(pack['seq_names'])},
              'overall': entry(list(range(S * K)))}
    lines = [' {:<16}'.format('sequence') + ''.join(' {:>10}'.format(c) for c in HOTA_SUMMARY_COLUMNS)]
    for name, e in list(result['sequences'].items()) + [('OVERALL', result['overall'])]:
        lines.append(' {:<16}'.format(str(name)[:16]) + ''.join(' {:>10.4f}'.format(e[c]) for c in HOTA_SUMMARY_COLUMNS))
    return result, ''.join(line + '\n' for line in lines)
