"""The host-emulation harness of the tests/test_*_emu.py: a csrc/su3_*.hip is compiled for the host with g++ against the
stand-in HIP header tests/native_host/emu/hip/hip_runtime.h (every thread of a workgroup an OS thread) and the shared
host side tests/native_host/emu/emu_host.hpp, under AddressSanitizer and UBSan, as the stand-alone program of
tests/native_host/<name>/<name>.cpp.  The program runs as a child process and talks through raw float64 files."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NH = os.path.join(ROOT, 'tests', 'native_host')


def build(tmp, name):
    """compile tests/native_host/<name>/<name>.cpp into the directory tmp; returns the executable"""
    exe = tmp / name
    subprocess.run(['g++', '-std=c++20', '-O1', '-g', '-pthread', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=undefined', '-I', os.path.join(NH, 'emu'),
                    '-I', os.path.join(ROOT, 'l2hmc-qcd_amd', 'csrc'), os.path.join(NH, name, name + '.cpp'),
                    '-o', str(exe)], check=True)
    return exe


def run(exe, args, inputs, nout):
    """exe args... in0 in1 ... out0 out1 ...: the arrays `inputs` (numpy or torch, real or complex float64) go to raw
    files next to exe, the program must succeed, and its nout raw outputs come back as flat float64 arrays"""
    fin = [str(exe.parent / f'in{i}.bin') for i in range(len(inputs))]
    fout = [str(exe.parent / f'out{i}.bin') for i in range(nout)]
    for f, a in zip(fin, inputs):
        np.ascontiguousarray(a.numpy() if hasattr(a, 'numpy') else a).view(np.float64).tofile(f)
    subprocess.run([str(exe), *map(str, args), *fin, *fout], check=True)
    return [np.fromfile(f) for f in fout]
