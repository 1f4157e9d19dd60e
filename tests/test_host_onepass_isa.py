"""The register budgets resample_onepass.hip's comments promise, read from the built object's metadata (no GPU needed).

The one-pass kernels share one chunk body and the phase functions; how the compiler allocates the result is not visible in the
source, and a spill in round 3's kernel is a vmcnt(0) behind its stores.  Numbers only: nothing here reads the instruction text."""
import os
import re
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "filterpy_amd", "csrc", "build", "resample_onepass.o")


def _kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import isa_lint
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    with tempfile.TemporaryDirectory() as tmp:
        return isa_lint.kernels(isa_lint.device_elf(OBJ, tmp))


def test_onepass_kernels_keep_their_register_budgets():
    if not os.path.exists(OBJ):
        pytest.skip("library not built here")
    ks = _kernels()
    # (mangled names: fk::resample_onepass_kernel<bool, bool, bool>, fk::resample_local_kernel<bool, int>, fk::resample_onepass2_kernel<int>)
    round3 = {n: k for n, k in ks.items() if re.search(r"resample_onepass_kernelILb[01]ELb[01]ELb[01]E", n)}
    local3 = {n: k for n, k in ks.items() if re.search(r"resample_local_kernelILb[01]ELi3E", n)}
    v2 = {int(re.search(r"resample_onepass2_kernelILi(\d+)E", n).group(1)): k for n, k in ks.items() if "resample_onepass2_kernelILi" in n}
    assert len(round3) == 8 and len(local3) == 2 and sorted(v2) == [5, 6, 7], sorted(ks)
    for n, k in round3.items():             # FK_OP_WAVES = 5 workgroups per CU: <= 96 VGPRs, no scratch
        assert int(k["scratch"]) == 0 and int(k["vgpr"]) <= 96, (n, k)
    for n, k in local3.items():             # three workgroups per CU run without a spill
        assert int(k["scratch"]) == 0, (n, k)
    for waves, budget in ((5, 96), (6, 80), (7, 72)):
        assert int(v2[waves]["vgpr"]) <= budget, (waves, v2[waves])
