"""The column-0 form of the rotation (qcp_lean_quaternion_col0, csrc/fc_kabsch_math.h) against the general form
(qcp_lean_quaternion_raw) on the host: tools/qcp_col0_check.cpp runs both on the same covariance, polynomial and eigenvalue
for more than 10^6 pairs -- 3 ... 416 atoms, rotation angles swept through the certificate's boundary (q0^2 from 0.5 to
0.7), arbitrary and small rotations, mirror images, near-duplicates -- and wherever column 0 certifies a pair the general
form must have picked column 0 and returned the same Q, nq and flag, bit for bit.  Built with the ROCm compiler for the host
only (the header takes its attributes from the HIP runtime header), with FMA contraction where the host has the
instruction: the header's fused regions then fuse as they do on the device."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return any(line.startswith("flags") and " fma " in line + " " for line in f)
    except OSError:
        return False


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc is needed: fc_kabsch_math.h includes the HIP runtime header")
    out = str(tmp_path_factory.mktemp("qcp_col0") / "qcp_col0_check")
    flags = ["-O2", "-std=c++17", "--offload-host-only", "-ffp-contract=off", "-Wall", "-Werror"] + (["-mfma"] if _host_has_fma() else [])
    r = subprocess.run([hipcc] + flags + ["-I", os.path.join(ROOT, "firecode_amd", "csrc"),
                                          os.path.join(ROOT, "tools", "qcp_col0_check.cpp"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def test_certified_pairs_have_the_general_forms_bits(checker):
    r = subprocess.run([checker], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    words = r.stdout.strip().splitlines()[-1].replace(",", "").split()
    cases, certified = int(words[0]), int(words[2])
    other_column, differing = int(words[4]), int(words[words.index("column") + 1])
    assert cases >= 10**6
    assert 0.3 * cases < certified < 0.8 * cases  # both sides of the certificate are exercised
    assert other_column == 0 and differing == 0
