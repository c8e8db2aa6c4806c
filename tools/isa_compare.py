#!/usr/bin/env python3
"""Device code of two source trees, kernel by kernel: for a refactor that must leave every kernel as it was.

  tools/isa_compare.py OLD_CSRC NEW_CSRC [--glob 'su3_*.hip'] [--cache DIR] [-j N]

Emits gfx950 assembly text for every source the glob matches in either directory (hipcc --cuda-device-only -S, the
flags of csrc/Makefile), splits it per kernel symbol and compares, for the union of the kernels of both trees
whichever file defines them: the instruction stream (comments, directives and blank lines stripped, the per-file
numbering of local labels removed) and the resource figures of the kernel's metadata.  Prints one line per kernel and
a summary; exit status 1 if any kernel differs or exists on one side only.  No GPU needed."""
import argparse
import concurrent.futures
import glob
import hashlib
import os
import re
import subprocess
import sys

FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '--cuda-device-only', '-S']
META = ('.vgpr_count', '.agpr_count', '.sgpr_count', '.private_segment_fixed_size', '.group_segment_fixed_size')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


def emit(src, out):
    if not os.path.exists(out):
        subprocess.run([HIPCC, *FLAGS, src, '-o', out], check=True)
    return out


def kernels(asm_path):
    """{symbol: (instruction lines, {metadata key: value})} of one assembly file"""
    text = open(asm_path).read()
    names = set(re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', text, re.M))
    body, cur = {}, None
    for line in text.split('\n'):
        m = re.match(r'^(\w+):', line)
        if m and m.group(1) in names:
            cur = body.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if re.match(r'^\.Lfunc_end\d+:', line):
            cur = None
            continue
        s = re.sub(r'\s*;.*$', '', line).strip()
        if not s or (s.startswith('.') and not s.endswith(':')):
            continue                                            # blank, comment or directive
        cur.append(re.sub(r'\.LBB\d+_', '.LBB_', re.sub(r'\s+', ' ', s)))
    meta, name, cur = {}, None, {}
    for line in text[text.find('amdhsa.kernels:'):].split('\n'):
        m = re.match(r'^\s*(?:- )?(\.\w+):\s*(\S+)\s*$', line)
        if not m:
            continue
        if m.group(1) == '.name':
            name = m.group(2)
        elif m.group(1) in META:
            cur[m.group(1)] = m.group(2)
        elif m.group(1) == '.wavefront_size':                   # (the last key of a kernel's record)
            meta[name], cur = cur, {}
    assert set(meta) == names == set(body), asm_path
    return {k: (body[k], meta[k]) for k in names}


def tree(csrc, pattern, cache, jobs):
    srcs = sorted(glob.glob(os.path.join(csrc, pattern)))
    tag = hashlib.sha1(os.path.abspath(csrc).encode()).hexdigest()[:8]
    os.makedirs(cache, exist_ok=True)
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        outs = list(ex.map(lambda s: emit(s, os.path.join(cache, f'{tag}_{os.path.basename(s)}.s')), srcs))
    found = {}
    for src, out in zip(srcs, outs):
        for k, v in kernels(out).items():
            assert k not in found, k
            found[k] = (os.path.basename(src), *v)
    return found


def demangle(names):
    r = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True)
    out = r.stdout.split('\n') if r.returncode == 0 else names
    return {n: re.sub(r'^void ', '', re.sub(r'\(.*$', '', d)) for n, d in zip(names, out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('old')
    ap.add_argument('new')
    ap.add_argument('--glob', default='su3_*.hip')
    ap.add_argument('--cache', default='/tmp/isa_compare')
    ap.add_argument('-j', type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    old, new = (tree(p, a.glob, a.cache, a.j) for p in (a.old, a.new))
    names = sorted(set(old) | set(new))
    short = demangle(names)
    bad = 0
    print(f'# {" ".join([os.path.basename(HIPCC), *FLAGS])}   sources: {a.glob}')
    print('# kernel | file (old -> new) | instructions | ' + ' '.join(k[1:] for k in META) + ' | verdict')
    for n in sorted(names, key=lambda n: ((new.get(n) or old[n])[0], short[n])):
        o, w = old.get(n), new.get(n)
        if o is None or w is None:
            bad += 1
            print(f'{short[n]} | {"only in the " + ("new" if o is None else "old") + " tree"} | DIFFERENT')
            continue
        same = o[1] == w[1] and o[2] == w[2]
        bad += not same
        files = o[0] if o[0] == w[0] else f'{o[0]} -> {w[0]}'
        figures = ' '.join(w[2][k] if o[2][k] == w[2][k] else f'{o[2][k]}->{w[2][k]}' for k in META)
        count = len(w[1]) if len(o[1]) == len(w[1]) else f'{len(o[1])}->{len(w[1])}'
        print(f'{short[n]} | {files} | {count} | {figures} | {"identical" if same else "DIFFERENT"}')
    print(f'# {len(names)} kernels, {len(names) - bad} identical, {bad} different')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
