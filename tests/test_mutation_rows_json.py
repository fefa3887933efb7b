"""The writer of a Mutations query's response text (lapis-silo_amd/host/mutation_rows_json.h) as a stand-alone program, built with
the address and undefined-behaviour sanitizers and run.  Its bytes are compared with one json::Value object per row and dump(),
ordered by a plain comparator: no row and one row; rows delivered in order, reversed and shuffled; two and twelve stores asked for
against their offset order, one twice, one without a row; count == total, an exponent, a count past 2^31; positions 1, 9, 10 and
29 903; the stop codon; a sequence name that needs escaping; every orderByFields key up and down, with ties, alone and together;
limit and offset inside, at and past the row count."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host_tools", "mutation_rows_json_main.cpp")
HOST = os.path.join(ROOT, "lapis-silo_amd", "host")


def test_writer_under_sanitizers(tmp_path):
    compiler = shutil.which("g++")
    if compiler is None:
        pytest.fail("g++ is needed to build the stand-alone program")
    program = str(tmp_path / "mutation_rows_json")
    subprocess.run(
        [compiler, "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-I", HOST, SOURCE, "-o", program],
        check=True, capture_output=True, text=True)
    done = subprocess.run([program], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "mutation rows json ok" in done.stdout
