"""One eager forward per shipped configuration on the GPU with ops.conv2d and the library's conv entry points wrapped.  Writes, as JSON:
'rows', one per distinct ops.conv2d call (layer, forms held, b3_min_rows -> the launchers that refused and the one that ran: the rows of
tests/golden/conv_routes.json, one per line there), and per configuration the ordered (entry point, scalar arguments) sequence of
the forward with its SHA-256 and the multiset of (dtype, numel) over graph.prepared_tensors(model).  Two trees compute the same
convolutions with the same kernels when their files are equal.  usage: tools/record_conv_routes.py OUT.json"""
import collections
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from mydetection_amd import _lib, graph, ops, synth
from mydetection_amd.models.general import name_to_model

FAMILY = {'mydet_conv3x3_p3_f32': 'conv_p3', 'mydet_conv2d_wino4_f32': 'conv_wino4', 'mydet_conv2d_wino_f32': 'conv_wino',
          'mydet_conv2d_igemm_b3_f32': 'conv_igemm_b3', 'mydet_conv2d_igemm_f32': 'conv_igemm'}
OTHER = ('mydet_conv1x1_upcat_f32', 'mydet_conv_stem_p3_f32', 'mydet_conv2d_stem_f32')
LD = {'conv_p3': (2, 1), 'conv_wino4': (3, 1), 'conv_wino': (3, 1), 'conv_igemm_b3': (3, 1), 'conv_igemm': (3, 1)}    # (ldy, ldr) among the ints

CONFIGS = [('yolov3_80', 32, 640), ('yolov3_80', 16, 640), ('yolov3_80', 1, 512), ('yolov3_80', 32, 512),
           ('efficientdet-d1', 16, 640), ('efficientdet-d1', 8, 640), ('d1_fcs2_atss', 32, 640), ('d1_fcs2_atss', 16, 640),
           ('ulo5m', 1, 256), ('ulo5m', 1, 640), ('rapid', 1, 256), ('rapid', 1, 1024), ('d1_rapid', 1, 256),
           ('d1_fcs2s', 1, 256), ('d1_fcs2s', 1, 640)]

SEQ = []


class Proxy:
    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in FAMILY and name not in OTHER:
            return fn

        def wrapped(*args):
            code = fn(*args)
            SEQ.append([name, [a for a in args if isinstance(a, int)], code])
            return code
        return wrapped


def main(path):
    real = _lib.lib()
    proxy = Proxy(real)
    _lib.lib = lambda: proxy
    rows = {}
    conv2d = ops.conv2d

    def recording_conv2d(x, w_ohwi, scale, shift, k, stride, pad, act, residual=None, out=None, out_ld=None, gate=None, wino=None,
                         wino4=None, interior=None, b3=None, b3_min_rows=None):
        n0 = len(SEQ)
        y = conv2d(x, w_ohwi, scale, shift, k, stride, pad, act, residual=residual, out=out, out_ld=out_ld, gate=gate, wino=wino,
                   wino4=wino4, interior=interior, b3=b3, b3_min_rows=b3_min_rows)
        calls = [c for c in SEQ[n0:] if c[0] in FAMILY]
        assert calls and calls[-1][2] == 0 and all(c[2] == -2 for c in calls[:-1]), calls
        fam = FAMILY[calls[-1][0]]
        ints = calls[-1][1]
        B, Cin, H, W = x.shape
        forms = sorted(n for n, t in (('wino', wino), ('wino4', wino4), ('b3', b3)) if t is not None)
        row = dict(B=B, H=H, W=W, Cin=Cin, Cout=int(w_ohwi.shape[0]), k=k, stride=stride, pad=list(pad), act=act, gated=gate is not None,
                   residual=residual is not None, ldy=ints[LD[fam][0]], ldr=ints[LD[fam][1]], forms=forms, b3_min_rows=b3_min_rows,
                   family=fam, refused=[FAMILY[c[0]] for c in calls[:-1]])
        rows[json.dumps(row, sort_keys=True)] = row
        return y

    ops.conv2d = recording_conv2d
    result = {'configs': {}}
    for name, B, size in CONFIGS:
        key = f'{name}_b{B}_{size}'
        m, cfg = name_to_model(name)
        m.load_state_dict(synth.make_state_dict(m.state_dict(), name), strict=True)
        m = m.eval().cuda()
        x = synth.make_image_set(0, B, size, cfg['general.input_format']).cuda()
        del SEQ[:]
        with torch.no_grad():
            if hasattr(m, 'forward_candidates'):
                m.forward_candidates(x)
            else:
                m(x)
        torch.cuda.synchronize()
        seq = [[n, a] for n, a, _ in SEQ]
        blob = json.dumps(seq).encode()
        seen, count = set(), collections.Counter()

        def walk(o):
            if isinstance(o, torch.Tensor):
                if id(o) not in seen:
                    seen.add(id(o))
                    count[f'{o.dtype}:{o.numel()}'] += 1
            elif isinstance(o, dict):
                for v in o.values():
                    walk(v)
            elif isinstance(o, (tuple, list)):
                for v in o:
                    walk(v)
        walk(graph.prepared_tensors(m))
        prepared = json.dumps(sorted(count.items())).encode()
        result['configs'][key] = dict(seq_len=len(seq), seq_sha256=hashlib.sha256(blob).hexdigest(), seq=seq,
                                      prepared_sha256=hashlib.sha256(prepared).hexdigest(), prepared_tensors=sum(count.values()),
                                      prepared=sorted(count.items()))
        print(key, len(seq), hashlib.sha256(blob).hexdigest()[:16], sum(count.values()), hashlib.sha256(prepared).hexdigest()[:16], flush=True)
        del m, x
        torch.cuda.empty_cache()
    result['rows'] = sorted(rows.values(), key=lambda r: json.dumps(r, sort_keys=True))
    print('rows', len(result['rows']), flush=True)
    with open(path, 'w') as f:
        json.dump(result, f)


if __name__ == '__main__':
    main(sys.argv[1])
