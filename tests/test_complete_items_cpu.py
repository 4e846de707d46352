"""The item tables of the complete alignments (csrc/fc_items.h, pure host code: no device needed): which (row blocks,
column tile) a workgroup takes.  tools/complete_items_check.cpp is compiled host-only and walks every table's items the
way the kernel does: over N in 17 ... 10 000, worlds 1, 2, 3, 8 (all ranks together), chunks of 1, 2, 4, 8 row blocks,
three tail lengths, both orders and the three tile widths

  * every (16-row tile, 16-column sub-tile) that touches the upper triangle with a real column is visited exactly once,
  * no sub-tile whose columns are all >= N is visited,

and the tables the prune screens share with it (chunk 1, every tile) are what the builder made before it knew chunks."""
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
    out = str(tmp_path_factory.mktemp("items") / "complete_items_check")
    r = subprocess.run(cxx + ["-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "firecode_amd", "csrc"),
                              os.path.join(ROOT, "tools", "complete_items_check.cpp"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_every_unit_of_the_triangle_once_and_no_padding(checker):
    r = subprocess.run([checker], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    configs, _, items, _, failures, _ = r.stdout.strip().splitlines()[-1].replace(",", "").split()
    assert int(failures) == 0 and int(configs) > 4000 and int(items) > 10 ** 6


def test_sizes_around_the_tile_edges(checker):
    """every N of a stretch that crosses row-block, tile and sub-tile edges (the default list has a few of each)"""
    r = subprocess.run([checker] + [str(n) for n in range(17, 400, 7)] + ["1023", "1024", "1025", "1039", "1040", "9999"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert r.stdout.strip().splitlines()[-1].endswith(" 0 failures")
