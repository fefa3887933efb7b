"""The texts of the 400 responses for malformed requests of MutationsPerSequence / AminoAcidMutationsPerSequence, byte for byte: the
GPU test of the actions asserts the status and that the field is named.  The program of tests/test_action_parse_messages.py
(tests/host_tools/parse_messages_main.cpp: one request per line through the JSON parser and the Action builders, `ok` or the
message per line) is linked here against the built engine library, without sanitizers, and run as its own process.  Parsing needs no
GPU."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "lapis-silo_amd", "host")
LIB = os.path.join(ROOT, "lapis-silo_amd", "lib")
TRUE = {"type": "True"}
NUC = "MutationsPerSequence action: the field sequenceName, if present, must be of type string"
AA = "AminoAcidMutationsPerSequence action: the field sequenceName, if present, must be of type string"
CASES = [
    ({"type": "MutationsPerSequence"}, "ok"),
    ({"type": "MutationsPerSequence", "sequenceName": "main"}, "ok"),
    ({"type": "MutationsPerSequence", "sequenceName": "S"}, "ok"),  # whether the name is one of a nucleotide sequence is the database's to say
    ({"type": "MutationsPerSequence", "orderByFields": ["substitutionCount", {"field": "missingPositions", "order": "descending"}], "limit": 3, "offset": 1}, "ok"),
    ({"type": "AminoAcidMutationsPerSequence", "sequenceName": "S"}, "ok"),
    ({"type": "MutationsPerSequence", "sequenceName": 5}, NUC),
    ({"type": "MutationsPerSequence", "sequenceName": 1.5}, NUC),
    ({"type": "MutationsPerSequence", "sequenceName": True}, NUC),
    ({"type": "MutationsPerSequence", "sequenceName": None}, NUC),
    ({"type": "MutationsPerSequence", "sequenceName": ["main"]}, NUC),
    ({"type": "MutationsPerSequence", "sequenceName": {"name": "main"}}, NUC),
    ({"type": "AminoAcidMutationsPerSequence", "sequenceName": 5}, AA),
    ({"type": "AminoAcidMutationsPerSequence", "sequenceName": ["S"]}, AA),
    ({"type": "AminoAcidMutationsPerSequence"}, "AminoAcidMutationsPerSequence action must contain the field sequenceName of type string (a gene)"),
    ({"type": "MutationsPerSequence", "limit": -1}, "If the action contains a limit, it must be a non-negative number"),
    ({"type": "MutationsPerSequence", "offset": "2"}, "If the action contains an offset, it must be a non-negative number"),
    ({"type": "MutationPerSequence"}, "MutationPerSequence is not a valid action"),
]


def test_parse_messages(built, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    program = str(tmp_path / "parse_messages")
    build = subprocess.run(
        ["g++", "-O1", "-std=c++20", "-I", os.path.join(ROOT, "include"), "-I", HOST, os.path.join(ROOT, "tests", "host_tools", "parse_messages_main.cpp"),
         "-o", program, "-L", LIB, "-lsilo_engine", "-lsilo_gpu", "-Wl,-rpath," + LIB, "-Wl,-rpath-link," + LIB, "-pthread"],
        capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    requests = "".join(json.dumps({"action": action, "filterExpression": TRUE}) + "\n" for action, _ in CASES)
    run = subprocess.run([program], input=requests.encode(), capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr.decode(errors="replace")[-3000:]
    got = run.stdout.decode().split("\n")
    assert got[-1] == "" and len(got) == len(CASES) + 1
    for (action, want), message in zip(CASES, got):
        assert message == want, action
