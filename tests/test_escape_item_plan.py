"""The host-side plan of a launch of k_scan_escapes_sliced (lapis-silo_amd/csrc/escape_item_plan.h: the items of a launch, the
order they are numbered in, the blocks that walk them) as a stand-alone program, built with the address and undefined-behaviour
sanitizers and run: 1 to 16 entries, 1, 2 and 512 slices, an entry without keys, grids of 1, n_items - 1, n_items and more blocks,
sums past 2^32.  It checks that every item is dealt exactly once and that the never-pruned items come first."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host_tools", "escape_item_plan_main.cpp")
CSRC = os.path.join(ROOT, "lapis-silo_amd", "csrc")


def test_plan_under_sanitizers(tmp_path):
    compiler = shutil.which("g++")
    if compiler is None:
        pytest.fail("g++ is needed to build the stand-alone program")
    program = str(tmp_path / "escape_item_plan")
    subprocess.run(
        [compiler, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-I", CSRC, SOURCE, "-o", program],
        check=True, capture_output=True, text=True)
    done = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "escape item plan ok" in done.stdout
