"""The texts of the 400 responses for malformed fields of the sequence-comparing actions (DistanceMatrix, Clusters,
MinimumSpanningTree, NearestAmong, NearestNeighbours, Haplotypes, Consensus and their amino-acid forms), byte for byte: the GPU
tests of these actions assert only the status.  A stand-alone program (tests/host_tools/parse_messages_main.cpp), built from the
host sources with AddressSanitizer + UndefinedBehaviorSanitizer and run as its own process, parses every line of
tests/golden/actionParseMessages/requests.jsonl and must print messages.txt, which was recorded before the parsers were folded
onto shared helpers.  Parsing needs no GPU.

The requests, per action: a well-formed one with and without every optional field; per field (sequenceName, maxDistance,
minComparedPositions, minClusterSize, neighbours, minDepth) the wrong types, -1, -2^31 - 1, 1.5, 5.0, 1e30, 2^31, 2^32 - 1, 2^32,
2^63 - 1, 2^63, 2^64 - 1, 0 where the minimum is 1, one past the maximum where there is one, both ends of the range, and the
field absent where it is required; the first i fields well-formed and all later ones malformed, for the order of the complaints;
NearestNeighbours with both, neither and each of primaryKey / sequence; NearestAmong's among as a non-object, an unknown type,
an empty object.  (2^63 and 2^64 - 1 answer ok as maxDistance of DistanceMatrix and NearestNeighbours, and nowhere else.)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "lapis-silo_amd", "host")
LIB = os.path.join(ROOT, "lapis-silo_amd", "lib")
GOLDEN = os.path.join(ROOT, "tests", "golden", "actionParseMessages")
NOT_NEEDED = ("c_api.cpp", "dataset_loader.cpp")  # the C ABI and the loader of data set directories: no part of parsing


def test_parse_messages_match_the_recorded_ones(built, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    sources = [os.path.join(HOST, name) for name in sorted(os.listdir(HOST)) if name.endswith(".cpp") and name not in NOT_NEEDED]
    program = str(tmp_path / "parse_messages")
    build = subprocess.run(
        ["g++", "-O1", "-g", "-std=c++20", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
         "-I", os.path.join(ROOT, "include"), "-I", HOST, os.path.join(ROOT, "tests", "host_tools", "parse_messages_main.cpp"), *sources,
         "-o", program, "-L", LIB, "-lsilo_gpu", "-Wl,-rpath," + LIB, "-pthread"],
        capture_output=True, text=True, timeout=900)
    if build.returncode != 0 and ("cannot find -lasan" in build.stderr or "libasan" in build.stderr):
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-3000:]
    with open(os.path.join(GOLDEN, "requests.jsonl"), "rb") as handle:
        requests = handle.read()
    with open(os.path.join(GOLDEN, "messages.txt"), "rb") as handle:
        expected = handle.read()
    run = subprocess.run([program], input=requests, capture_output=True, timeout=900, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    stderr = run.stderr.decode(errors="replace")
    assert run.returncode == 0, stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in stderr and "runtime error" not in stderr, stderr[-3000:]
    got_lines, expected_lines, request_lines = run.stdout.split(b"\n"), expected.split(b"\n"), requests.split(b"\n")
    assert len(request_lines) > 300 and expected_lines.count(b"ok") >= 9  # the fixture is the whole one
    for request, got, want in zip(request_lines, got_lines, expected_lines):
        assert got == want, request.decode()
    assert run.stdout == expected
