"""The texts of the 400 responses for malformed DistinctSequenceCounts actions, byte for byte.  The program of
tests/test_action_parse_messages.py (tests/host_tools/parse_messages_main.cpp: one request per line through the JSON parser and the
Expression and Action builders, `ok` or the message per line) is linked here against the built engine library, without sanitizers,
and run as its own process.  Parsing needs no GPU.  The messages for a sequence the database does not have and for a sharded database
come from executing the action against a database: tests/test_distinct_sequence_counts_gpu.py compares them, byte for byte as well,
with UNKNOWN_SEQUENCE and SHARDED below."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "lapis-silo_amd", "host")
LIB = os.path.join(ROOT, "lapis-silo_amd", "lib")
OK = {"type": "DistinctSequenceCounts"}
NAME = "DistinctSequenceCounts action: the field sequenceName, if present, must be of type string"
MIN_COUNT = "DistinctSequenceCounts action: the field minCount, if present, must be an integer of at least 1"
MAX_CLASSES = "DistinctSequenceCounts action: the field maxClasses, if present, must be an integer from 1 to 16384"
UNKNOWN_SEQUENCE = "DistinctSequenceCounts: the field sequenceName: Database does not contain a sequence with name: '{}'"
SHARDED = ("DistinctSequenceCounts is not supported on a sharded database yet: the rows of a selection on the other ranks take part in "
           "the choice, and a row's number in the database is not known to a rank")


def _order_by(value):
    return ("The orderByField '" + json.dumps(value, separators=(",", ":")) + "' must be either a string or an object containing the fields "
            "'field':string and 'order':string, where the value of order is 'ascending' or 'descending'")


CASES = [
    (OK, "ok"),
    (dict(OK, sequenceName="S"), "ok"),
    (dict(OK, sequenceName="no such sequence"), "ok"),  # (known only to a database)
    (dict(OK, minCount=1, maxClasses=1), "ok"),
    (dict(OK, minCount=2 ** 31 - 1, maxClasses=16384), "ok"),
    (dict(OK, orderByFields=["count", {"field": "primaryKey", "order": "descending"}], limit=3, offset=1), "ok"),
    (dict(OK, orderByFields=["distance"]), "ok"),  # (refused when the action runs: the fields of its rows)
    (dict(OK, sequenceName=5), NAME),
    (dict(OK, sequenceName=None), NAME),
    (dict(OK, sequenceName=["S"]), NAME),
    (dict(OK, minCount=0), MIN_COUNT),
    (dict(OK, minCount=-1), MIN_COUNT),
    (dict(OK, minCount=1.5), MIN_COUNT),
    (dict(OK, minCount="2"), MIN_COUNT),
    (dict(OK, minCount=None), MIN_COUNT),
    (dict(OK, minCount=2 ** 31), MIN_COUNT),
    (dict(OK, minCount=[1]), MIN_COUNT),
    (dict(OK, maxClasses=0), MAX_CLASSES),
    (dict(OK, maxClasses=16385), MAX_CLASSES),
    (dict(OK, maxClasses=-3), MAX_CLASSES),
    (dict(OK, maxClasses="all"), MAX_CLASSES),
    (dict(OK, maxClasses=None), MAX_CLASSES),
    (dict(OK, maxClasses=10.0), MAX_CLASSES),
    (dict(OK, minCount=0, maxClasses=0), MIN_COUNT),
    (dict(OK, sequenceName=1, minCount=0), NAME),
    (dict(OK, orderByFields=[3]), _order_by(3)),
    (dict(OK, orderByFields=[{"field": "count", "order": "down"}]), _order_by({"field": "count", "order": "down"})),
    (dict(OK, limit=-1), "If the action contains a limit, it must be a non-negative number"),
    (dict(OK, offset="1"), "If the action contains an offset, it must be a non-negative number"),
    ({"type": "DistinctSequencesCounts"}, "DistinctSequencesCounts is not a valid action"),
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
    requests = "".join(json.dumps({"action": action, "filterExpression": {"type": "True"}}) + "\n" for action, _ in CASES)
    run = subprocess.run([program], input=requests.encode(), capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr.decode(errors="replace")[-3000:]
    got = run.stdout.decode().split("\n")
    assert got[-1] == "" and len(got) == len(CASES) + 1
    for (action, want), message in zip(CASES, got):
        assert message == want, action
