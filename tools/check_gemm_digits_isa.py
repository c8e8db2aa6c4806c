#!/usr/bin/env python3
"""Static check of the hand-counted waits of csrc/gemm_digits.hip (hipcc cross-compiles without a GPU), on the ISA
of gemm_digits_kernel:
  - no spills, and no vector-memory instruction other than LDS-DMA before the epilogue (a spill or a compiler
    load would shift the hand-counted vmcnt);
  - loaders: every `s_waitcnt vmcnt(N)` in front of an `s_barrier` has N = 0, or N = 7 with at least 14 LDS-DMA
    pieces issued since the previous barrier (the seven activation pieces of the slab the barrier completes, then
    the seven weight pieces of the slab after it: pieces retire in order, so only the latter stay in flight);
  - matrix wavefronts: per slab 28 ds_read_b128 and 112 MFMAs (+ 12: the deferred rows appear twice), and no MFMA reads a register whose ds_read_b128
    a counted `s_waitcnt lgkmcnt(N)` has not retired yet (LDS returns in order: lgkmcnt(N) leaves the last N).
usage: check_gemm_digits_isa.py  -> exit code 0 / 1"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'l2hmc-qcd_amd', 'csrc')
KERNEL = 'gemm_digits_kernel'          # (found by this part of its mangled name)


def isa() -> str:
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, 'gd.s')
        subprocess.run(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC',
                        '-I' + os.path.join(ROOT, 'include'), '-I' + CSRC, '-S', '--cuda-device-only', '-o', out,
                        os.path.join(CSRC, 'gemm_digits.hip')], check=True, stderr=subprocess.DEVNULL)
        return open(out).read()


def regs(tok: str):
    """'v[10:13],' -> {10..13}; 'v5,' -> {5}; anything else -> empty"""
    m = re.match(r'^v\[(\d+):(\d+)\]', tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r'^v(\d+)\b', tok)
    return {int(m.group(1))} if m else set()


def check(text: str):
    body = text[re.search(r'^\w*' + KERNEL + r'\w*:', text, re.M).start():]
    body = body[:body.index('.Lfunc_end')]
    meta = text[re.search(r'\.name:\s+\w*' + KERNEL, text).start():]
    spill = int(re.search(r'\.vgpr_spill_count:\s*(\d+)', meta).group(1))
    vgpr = int(re.search(r'\.vgpr_count:\s*(\d+)', meta).group(1))
    errors = []
    if spill:
        errors.append(f'{spill} spilled VGPRs')
    dma_since, loader_waits = 0, []
    outstanding = []                  # destination register sets of the ds_read_b128 in flight, oldest first
    reads = mfmas = 0
    per_slab = []
    seen_mfma = False
    lines = body.split('\n')
    bars = [i for i, l in enumerate(lines) if l.strip().startswith('s_barrier')]
    for i, line in enumerate(lines):
        t = line.strip().split()
        if not t or t[0].startswith((';', '.')):
            continue
        op = t[0]
        if op.startswith('global_load_lds'):
            dma_since += 1
        elif op.startswith(('global_', 'scratch_', 'buffer_', 'flat_')) and bars[0] < i < bars[-1]:
            errors.append('vector-memory instruction beside the LDS-DMA: ' + line.strip())
        elif op == 'ds_read_b128':
            outstanding.append(regs(t[1]))
            reads += 1
        elif op.startswith('v_mfma'):
            seen_mfma = True
            mfmas += 1
            src = regs(t[2]) | regs(t[3])
            if any(src & d for d in outstanding):
                errors.append('MFMA reads a fragment whose ds_read_b128 is not retired: ' + line.strip())
        elif op == 's_waitcnt':
            m = re.search(r'lgkmcnt\((\d+)\)', line)
            if m:
                n = int(m.group(1))
                outstanding = outstanding[len(outstanding) - n:] if n else []
            m = re.search(r'vmcnt\((\d+)\)', line)
            if m:
                loader_waits.append((int(m.group(1)), dma_since))
        elif op == 's_barrier':
            if loader_waits and loader_waits[-1][1] == dma_since and dma_since:
                n, since = loader_waits[-1]
                if n not in (0, 7) or (n == 7 and since < 14):
                    errors.append(f'vmcnt({n}) in front of a barrier with {since} LDS-DMA pieces since the last one')
                if n == 0:
                    # (the barrier of the LAST slab, everything drained: hipcc lays this exit path out between the
                    # activation and the weight pieces of the steady-state period, which it does not interrupt)
                    continue
            dma_since = 0
            if seen_mfma:
                per_slab.append((reads, mfmas))
            reads = mfmas = 0
    # the loop body runs from one barrier of the matrix wavefronts to the next: the pieces of the body in program
    # order (the range flush sits in a branch of its own) add up to one slab
    total_reads = sum(r for r, _ in per_slab) + reads
    total_mfma = sum(m for _, m in per_slab) + mfmas
    report = (f'gemm_digits_kernel: {vgpr} VGPRs, {spill} spills, {total_reads} ds_read_b128, {total_mfma} MFMAs, '
              f'{body.count("global_load_lds")} LDS-DMA pieces, loader waits {sorted(set(w for w, _ in loader_waits))}')
    # 112 MFMAs per slab + the 12 of the deferred rows a second time (after the barrier / in the range flush)
    if (total_reads, total_mfma) != (28, 124):
        errors.append(f'expected 28 ds_read_b128 and 124 MFMAs in the slab loop, found {total_reads} and {total_mfma}')
    if not any(w == 7 for w, _ in loader_waits):
        errors.append('no vmcnt(7) found: the loaders drain their weight pieces at every barrier')
    return errors, report, (total_reads, total_mfma)


if __name__ == '__main__':
    errs, rep, _ = check(isa())
    print(rep)
    for e in errs:
        print('  ' + e)
    sys.exit(1 if errs else 0)
