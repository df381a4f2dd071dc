"""CPU check of the test-only probe library (madigan_amd/build.py
build_math_probe, tests/csrc/mgn_math_probe.hip): build() leaves it outside the
product, under tests/_probe, built from the source as it is now and exporting
the entries tests/test_gpu_math_probe.py calls.  Skips as tests/test_build.py
does where there is no ROCm toolchain or build() has not run."""
import ctypes
import os
import re

import pytest

from madigan_amd import build as B


def test_math_probe_built_with_its_entries():
    try:
        B.hipcc()
    except RuntimeError as e:
        pytest.skip(f"no ROCm toolchain here: {e}")
    if not os.path.exists(B.OUT):
        pytest.skip("the library has not been built")
    assert os.path.exists(B.PROBE_OUT), f"{B.PROBE_OUT} missing after build()"
    assert os.path.commonpath([B.PROBE_OUT, B.OBJ]) != B.OBJ  # (_obj holds intermediates only)
    assert B.PROBE_SRC not in B.sources() and B.PROBE_SRC not in B.deps()
    probe = ctypes.CDLL(B.PROBE_OUT)
    for name in B.PROBE_ENTRIES:
        assert hasattr(probe, name), f"the probe does not export {name}"
    # built from the source as it is now: the source states its entries' version
    with open(B.PROBE_SRC) as f:
        abi = int(re.search(r"int mgp_abi\(void\) \{ return (\d+); \}", f.read()).group(1))
    assert probe.mgp_abi() == abi, "the probe library is older than its source"
    product = ctypes.CDLL(B.OUT)
    for name in B.PROBE_ENTRIES:
        assert not hasattr(product, name), f"the product library exports {name}"
