"""csrc/gemm_digits.hip counts its own waits (vmcnt in the loaders, lgkmcnt in the matrix wavefronts): the static
check of tools/check_gemm_digits_isa.py on the ISA hipcc emits here (cross-compiled, no GPU needed)."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gemm_digits_waits_are_sound():
    spec = importlib.util.spec_from_file_location('check_gemm_digits_isa',
                                                  os.path.join(ROOT, 'tools', 'check_gemm_digits_isa.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    errors, report, _ = mod.check(mod.isa())
    assert not errors, (report, errors)
