"""The layout of Xt, the row-tile-major copy of the ensemble the atom pass of the complete alignments reads (csrc/fc_items.h:
row_tile_offset, pure host code: no device needed).  tools/row_tiles_check.cpp is compiled host-only and walks the buffer the
way a wave does, over N = 1 ... 40 conformers and A = 1 ... 9 atoms:

  * every (row, atom, coordinate) has an offset of its own inside the buffer,
  * the 16-byte pieces the lanes load hold exactly the two atoms of a round for the lane's row,
  * padding rows and the padding atom of an odd A fall where the kernel expects zeros, and with the real elements they fill
    the buffer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_compiler():
    for name in ("c++", "g++", "clang++"):
        path = shutil.which(name)
        if path:
            return [path]
    for path in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if os.path.exists(path):
            return [path]
    return None


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("row_tiles") / "row_tiles_check")
    r = subprocess.run(cxx + ["-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "firecode_amd", "csrc"),
                              os.path.join(ROOT, "tools", "row_tiles_check.cpp"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_every_element_once_and_zeros_where_the_kernel_expects_them(checker):
    r = subprocess.run([checker], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    configs, _, elements, _, failures, _ = r.stdout.strip().splitlines()[-1].replace(",", "").split()
    assert int(failures) == 0 and int(configs) == 40 * 9
    assert int(elements) == sum(n * a * 3 for n in range(1, 41) for a in range(1, 10))


def test_sizes_around_the_tile_edges(checker):
    """N around the 16-row tile and the 64-row padding, and a size with many tiles"""
    r = subprocess.run([checker] + [str(n) for n in (15, 16, 17, 63, 64, 65, 127, 129, 1041)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert r.stdout.strip().splitlines()[-1].endswith(" 0 failures")
