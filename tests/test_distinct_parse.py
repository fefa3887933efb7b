"""The texts of the 400 responses for malformed DistinctSequences filter expressions, byte for byte.  The program of
tests/test_action_parse_messages.py (tests/host_tools/parse_messages_main.cpp: one request per line through the JSON parser and the
Expression and Action builders, `ok` or the message per line) is linked here against the built engine library, without sanitizers,
and run as its own process.  Parsing needs no GPU.  The message for a sequence the database does not have comes from compiling the
expression against a database: tests/test_distinct_gpu.py compares it, byte for byte as well, with UNKNOWN_SEQUENCE below."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "lapis-silo_amd", "host")
LIB = os.path.join(ROOT, "lapis-silo_amd", "lib")
TRUE = {"type": "True"}
OK = {"type": "DistinctSequences", "child": TRUE}
CHILD = "The field 'child' in a DistinctSequences expression needs to be an object"
NAME = "The field 'sequenceName' in a DistinctSequences expression, if present, needs to be a string"
UNKNOWN_SEQUENCE = "DistinctSequences: the field sequenceName: Database does not contain a sequence with name: '{}'"
SHARDED = ("DistinctSequences is not supported on a sharded database yet: the rows of a selection on the other ranks take part in "
           "the choice, and a row's number in the database is not known to a rank")

CASES = [
    (OK, "ok"),
    (dict(OK, sequenceName="S"), "ok"),
    (dict(OK, sequenceName="no such sequence"), "ok"),  # (known only to a database)
    (dict(OK, child=dict(OK, sequenceName="main")), "ok"),
    (dict(OK, child={"type": "Sample", "child": OK, "size": 3}), "ok"),
    ({"type": "Sample", "child": OK, "size": 3}, "ok"),
    ({"type": "DistinctSequences"}, "The field 'child' is required in a DistinctSequences expression"),
    ({"type": "DistinctSequences", "sequenceName": "S"}, "The field 'child' is required in a DistinctSequences expression"),
    (dict(OK, child="True"), CHILD),
    (dict(OK, child=[TRUE]), CHILD),
    (dict(OK, child=None), CHILD),
    (dict(OK, child=3), CHILD),
    (dict(OK, child={"type": "Nothing"}), "Unknown object filter type 'Nothing'"),
    (dict(OK, child={}), "The field 'type' is required in any filter expression"),
    (dict(OK, sequenceName=5), NAME),
    (dict(OK, sequenceName=None), NAME),
    (dict(OK, sequenceName=["S"]), NAME),
    (dict(OK, child=dict(OK, sequenceName=True)), NAME),
    ({"type": "And", "children": [TRUE, {"type": "DistinctSequences"}]}, "The field 'child' is required in a DistinctSequences expression"),
    ({"type": "Not", "child": {"type": "Maybe", "child": dict(OK, child="x")}}, CHILD),
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
    requests = "".join(json.dumps({"action": {"type": "Aggregated"}, "filterExpression": expression}) + "\n" for expression, _ in CASES)
    run = subprocess.run([program], input=requests.encode(), capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr.decode(errors="replace")[-3000:]
    got = run.stdout.decode().split("\n")
    assert got[-1] == "" and len(got) == len(CASES) + 1
    for (expression, want), message in zip(CASES, got):
        assert message == want, expression
