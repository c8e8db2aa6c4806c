"""Device code, parent against this commit: from the assembly of su3_wilson.hip, su3_wilson_eo.hip and
su3_wilson_force.hip of two checkouts,
    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -I include FILE.hip -o DIR/FILE.s
print per kernel the instruction count, the counts of vector-memory and of v_fma_f64 / v_mul_f64 / v_add_f64
instructions, the register counts and scratch size of the metadata, a verdict, and every differing line.

    python profiles/wilson_hop_single_source/isa_compare.py PARENT_DIR HEAD_DIR"""
import difflib
import re
import sys

FILES = ('su3_wilson', 'su3_wilson_eo', 'su3_wilson_force')
META = ('.vgpr_count', '.agpr_count', '.sgpr_count', '.private_segment_fixed_size')


def kernels(path):
    """{kernel: (instruction lines, metadata)}"""
    text = open(path).read()
    out = {}
    for m in re.finditer(r'^(_ZN3l2q\w+):[^\n]*\n(.*?)^\s+s_endpgm', text, re.S | re.M):
        body = [ln.split(';')[0].strip() for ln in m.group(2).split('\n')]
        out[m.group(1)] = [ln for ln in body if ln and not ln.startswith('.') and not ln.endswith(':')] + ['s_endpgm']
    meta = {}
    for blk in text.split('  - .agpr_count:')[1:]:
        blk = '.agpr_count:' + blk
        name = re.search(r'\.name:\s+(\S+)', blk).group(1)
        meta[name] = [int(re.search(re.escape(k) + r':\s+(\d+)', blk).group(1)) for k in META]
    return {k: (v, meta[k]) for k, v in out.items()}


def count(ins, *prefixes):
    return sum(i.startswith(prefixes) for i in ins)


def main(pdir, hdir):
    print('# kernel | file | instructions parent -> head | vector-memory | v_fma_f64 v_mul_f64 v_add_f64 | '
          'vgpr_count agpr_count sgpr_count private_segment_fixed_size | verdict')
    diffs = []
    for f in FILES:
        kp, kh = kernels(f'{pdir}/{f}.s'), kernels(f'{hdir}/{f}.s')
        assert sorted(kp) == sorted(kh)
        for k in kp:
            (ip, mp), (ih, mh) = kp[k], kh[k]
            vm = [count(i, 'global_', 'flat_', 'buffer_', 'scratch_') for i in (ip, ih)]
            fp = [[count(i, op) for op in ('v_fma_f64', 'v_mul_f64', 'v_add_f64')] for i in (ip, ih)]
            d = [ln for ln in difflib.unified_diff(ip, ih, lineterm='', n=0) if ln[0] in '+-' and ln[:3] not in ('+++', '---')]
            same_counts = vm[0] == vm[1] and fp[0] == fp[1] and mp[0] == mh[0] and mp[3] == mh[3] == 0
            verdict = 'identical' if ip == ih and mp == mh else \
                f"{len(d)} differing lines; counts {'equal' if same_counts else 'DIFFER'}"
            show = lambda a, b: f'{a}' if a == b else f'{a} -> {b}'
            print(f"{k} | {f}.hip | {show(len(ip), len(ih))} | {show(vm[0], vm[1])} | "
                  f"{show(' '.join(map(str, fp[0])), ' '.join(map(str, fp[1])))} | "
                  f"{show(' '.join(map(str, mp)), ' '.join(map(str, mh)))} | {verdict}")
            if d:
                diffs.append((k, d))
    for k, d in diffs:
        print(f'\n# {k}: every differing line (- parent, + head)')
        print('\n'.join(d))


if __name__ == '__main__':
    main(*sys.argv[1:3])
