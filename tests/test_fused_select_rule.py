"""The host-side rule of silo_gpu_mutations_scan_select (lapis-silo_amd/csrc/fused_select_rule.h: do the ranges of a call tile a
filter's count table; how many blocks of the finish launches take a ticket) as a stand-alone program, built with the address and
undefined-behaviour sanitizers and run: 1, 16 and 17 ranges, gaps and overlaps in the tiling, sums past 2^32."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host_tools", "fused_select_rule_main.cpp")
CSRC = os.path.join(ROOT, "lapis-silo_amd", "csrc")


def test_rule_under_sanitizers(tmp_path):
    compiler = shutil.which("g++")
    if compiler is None:
        pytest.fail("g++ is needed to build the stand-alone program")
    program = str(tmp_path / "fused_select_rule")
    subprocess.run(
        [compiler, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-I", CSRC, SOURCE, "-o", program],
        check=True, capture_output=True, text=True)
    done = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "fused select rule ok" in done.stdout
