"""The speed record as a table: from the files of the alternating runs (`-- parent` / `-- head` sections holding the
output of tools/bench_wilson.py --kernels --eo --propagator and tools/bench_wilson_force.py --trajectory with and
without --even-odd, which runs the full-lattice trajectory again beside the even-odd one) take every figure in ms, in the order taken, and say whether each figure of this commit lies inside
the parent's own min - max of that session, below it or above it.

    python profiles/wilson_hop_single_source/speed_table.py ROUND_FILE..."""
import re
import sys

PAT = [(re.compile(r'^(\S[^\n]*?)\s{2,}([\d.]+) ms \(min'), None),                       # a kernel line: the median
       (re.compile(r'^(wilson_solve\w+)\s+([\d.]+) ms'), None),
       (re.compile(r'^(thin links|one HYP step): kappa [\d.]+: ([\d.]+) ms'), 'propagator, '),
       (re.compile(r'^(one leapfrog) \(.*?\): ([\d.]+) ms wall'), None),
       (re.compile(r'^\d+ (trajectories) x .* median wall ([\d.]+) ms'), None)]


def runs(paths):
    """[(side, {label: ms})] in the order taken; a label is the line's name and which time it occurs in the run"""
    out = []
    for p in paths:
        for sec in open(p).read().split('-- ')[1:]:
            side, vals, seen, eo = sec.split('\n', 1)[0].strip(), {}, {}, False
            for ln in sec.split('\n')[1:]:
                eo = ln.rstrip().endswith('even_odd True') if 'even_odd ' in ln else eo      # the trajectory tool's header
                for pat, pre in PAT:
                    m = pat.match(ln.strip() if pre is None and not ln.startswith(' ') else ln)
                    if m and not ln.startswith(' '):
                        name = (pre or '') + m.group(1) + (', even-odd' if eo and m.group(1) in ('one leapfrog', 'trajectories') else '')
                        seen[name] = seen.get(name, 0) + 1
                        vals[f'{name} #{seen[name]}'] = float(m.group(2))
                        break
            out.append((side, vals))
    return out


def main(paths):
    rs = runs(paths)
    print('order taken: ' + ', '.join(s for s, _ in rs))
    print('figure | parent, ms | this commit, ms | parent min - max | this commit against it')
    above = 0
    for label in rs[0][1]:
        par = [v[label] for s, v in rs if s == 'parent']
        head = [v[label] for s, v in rs if s == 'head']
        lo, hi = min(par), max(par)
        word = ', '.join('above' if h > hi else 'below' if h < lo else 'inside' for h in head)
        above += sum(h > hi for h in head)
        print(f"{label} | {', '.join(map(str, par))} | {', '.join(map(str, head))} | {lo} - {hi} | {word}")
    print(f'{len(rs[0][1])} figures; figures of this commit above the parent\'s maximum: {above}')


if __name__ == '__main__':
    main(sys.argv[1:])
