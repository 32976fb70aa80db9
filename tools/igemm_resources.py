"""Host only: the kernels of csrc/conv_igemm.hip in two builds of libmydet_hip.so, side by side -- names, registers, scratch, static
LDS (code object metadata) and whether the instruction streams are the same.

    python tools/igemm_resources.py OLD.so NEW.so [--out FILE.json] [--mark KERNEL ...]

--mark names a kernel of another source file instead: the kernels of every code object that holds one of the marks are compared
(profiles/paint_tile.md: --mark draw_rgb_kernel --mark redact_paint_kernel).

Exit code 1 when the kernel lists differ or a kernel without scratch gained some.  Used for profiles/igemm_frame.md.
"""
import argparse
import hashlib
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_store_hazard import code_objects, instructions             # noqa: E402

FIELDS = ('vgpr_count', 'agpr_count', 'sgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size')
MARK = 'conv_igemm_b3w_kernel'            # a kernel only conv_igemm.hip has: finds its code object


def kernels(lib, marks=(MARK,)):
    """{kernel name: {field: value, 'isa': digest of its instructions}} of the code objects that hold a kernel of `marks`."""
    found = {}
    for (_, notes), (_, dis) in zip(code_objects(lib, notes=True), code_objects(lib)):
        if not any(m in notes for m in marks):
            continue
        out, cur = {}, None
        for line in notes.splitlines():
            m = re.match(r'\s*(?:- )?\.(\w+):\s+(\S+)', line)
            if not m:
                continue
            if m.group(1) == 'agpr_count':                   # the first field of a kernel's record
                cur = {}
            if cur is not None and m.group(1) in FIELDS:
                cur[m.group(1)] = int(m.group(2))
            if cur is not None and m.group(1) == 'name':
                out[m.group(2)] = cur
        isa = {}
        for fn, ins in instructions(dis):
            # branch targets and literal addresses move with the code's position in the object: keep the mnemonic and register operands
            isa.setdefault(fn, hashlib.sha1()).update((re.sub(r'\b(0x)?[0-9a-f]{4,}\b|<[^>]*>', '', ins) + '\n').encode())
        for name, rec in out.items():
            rec['isa'] = isa[name].hexdigest() if name in isa else None
        found.update(out)
    if not found:
        raise SystemExit(f'{lib}: no code object with {marks}')
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('old')
    ap.add_argument('new')
    ap.add_argument('--out')
    ap.add_argument('--mark', action='append', help='a kernel name that finds a code object (default: the one of conv_igemm.hip)')
    args = ap.parse_args()
    marks = tuple(args.mark or (MARK,))
    old, new = kernels(args.old, marks), kernels(args.new, marks)
    res = {'only_old': sorted(set(old) - set(new)), 'only_new': sorted(set(new) - set(old)), 'kernels': len(old), 'differ': {},
           'same_isa': 0, 'gained_scratch': []}
    for name in sorted(set(old) & set(new)):
        a, b = old[name], new[name]
        res['same_isa'] += a['isa'] == b['isa']
        if any(a[f] != b[f] for f in FIELDS):
            res['differ'][name] = {f: [a[f], b[f]] for f in FIELDS}
        if a['private_segment_fixed_size'] == 0 and b['private_segment_fixed_size'] > 0:
            res['gained_scratch'].append(name)
    res['scratch_old'] = {n: r['private_segment_fixed_size'] for n, r in old.items() if r['private_segment_fixed_size']}
    res['table'] = {n: {f: [old[n][f], new[n][f]] for f in FIELDS} for n in sorted(set(old) & set(new))}
    print(json.dumps({k: v for k, v in res.items() if k != 'table'}, indent=1))
    if args.out:
        json.dump(res, open(args.out, 'w'), indent=1)
    return 1 if res['only_old'] or res['only_new'] or res['gained_scratch'] else 0


if __name__ == '__main__':
    sys.exit(main())
