"""CPU checks of the device headers' structure (madigan_amd/csrc/*.h, one
subject per header: DESIGN.md section 4): every header compiles as a
translation unit of its own, with the product's flags, so it includes what it
uses; the three-role kernel's header does not reach its helpers through the
two-role kernel's, the launch declarations include no kernel, and no header
forward-declares broker_spec (mgn_kernels.h once did, for a definition that
lived in a header including it)."""
import glob
import os
import re
import subprocess

import pytest

from madigan_amd import build as B

HEADERS = sorted(os.path.basename(h) for h in glob.glob(os.path.join(B.CSRC, "*.h")))


def _includes(header):
    with open(os.path.join(B.CSRC, header)) as f:
        return set(re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), re.M))


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_alone(header, tmp_path):
    try:
        cc = B.hipcc()
    except RuntimeError as e:
        pytest.skip(f"no ROCm toolchain here: {e}")
    src = tmp_path / "t.hip"
    src.write_text(f'#include "{header}"\n')
    r = subprocess.run([cc, *B.FLAGS, f"-I{B.CSRC}", "-fsyntax-only", "-Werror",
                        "-Wno-unused-command-line-argument", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_kernel_headers_stay_apart():
    assert "mgn_duo.h" not in _includes("mgn_trio.h")
    assert not _includes("mgn_launch.h") & {"mgn_kernels.h", "mgn_duo.h", "mgn_trio.h"}


@pytest.mark.parametrize("header", HEADERS)
def test_no_forward_declaration_of_broker_spec(header):
    with open(os.path.join(B.CSRC, header)) as f:
        text = f.read()
    assert not re.search(r"\bvoid\s+broker_spec\s*\([^;{]*\)\s*;", text)
