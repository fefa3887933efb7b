"""The texts of the 400 responses for malformed Sample filter expressions, byte for byte: the GPU test of the expression asserts the
status and that the field is named.  The program of tests/test_action_parse_messages.py (tests/host_tools/parse_messages_main.cpp:
one request per line through the JSON parser and the Expression and Action builders, `ok` or the message per line) is linked here
against the built engine library, without sanitizers, and run as its own process.  Parsing needs no GPU."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "lapis-silo_amd", "host")
LIB = os.path.join(ROOT, "lapis-silo_amd", "lib")
TRUE = {"type": "True"}
OK = {"type": "Sample", "child": TRUE, "size": 300}
WEEK = {"dateFrom": "2021-01-04", "dateTo": "2021-01-10"}
NEXT_WEEK = {"dateFrom": "2021-01-11", "dateTo": "2021-01-17"}
SIZE = "The field 'size' in a Sample expression needs to be a non-negative integer"
SEED = "The field 'seed' in a Sample expression, if present, needs to be a non-negative integer"
TOGETHER = "The fields 'dateField' and 'dateRanges' in a Sample expression need to be given together"
RANGES = ("The field 'dateRanges' in a Sample expression needs to be an array of objects "
          "{\"dateFrom\": string or null, \"dateTo\": string or null}")
OVERLAP = "The date ranges in a Sample expression overlap; each row may fall in at most one"


def _strata(*ranges, **fields):
    return {**OK, "dateField": "date", "dateRanges": list(ranges), **fields}


CASES = [
    (OK, "ok"),
    (dict(OK, size=0), "ok"),
    (dict(OK, size=2 ** 31 - 1, seed=2 ** 63 - 1), "ok"),
    (dict(OK, seed=0), "ok"),
    (dict(OK, child=dict(OK, seed=3)), "ok"),
    (_strata(), "ok"),
    (_strata(WEEK, NEXT_WEEK), "ok"),
    (_strata(NEXT_WEEK, WEEK), "ok"),
    (_strata({"dateFrom": None, "dateTo": "2021-01-03"}, WEEK, {"dateFrom": "2021-01-11"}), "ok"),
    (_strata({}), "ok"),  # one range that is open at both ends
    (_strata(*[{"dateFrom": f"{2000 + k // 12}-{k % 12 + 1:02d}-01", "dateTo": f"{2000 + k // 12}-{k % 12 + 1:02d}-02"} for k in range(1024)]), "ok"),
    ({"type": "Sample", "size": 3}, "The field 'child' is required in a Sample expression"),
    (dict(OK, child="True"), "The field 'child' in a Sample expression needs to be an object"),
    (dict(OK, child=[TRUE]), "The field 'child' in a Sample expression needs to be an object"),
    (dict(OK, child=None), "The field 'child' in a Sample expression needs to be an object"),
    (dict(OK, child={"type": "Nothing"}), "Unknown object filter type 'Nothing'"),
    (dict(OK, child={}), "The field 'type' is required in any filter expression"),
    ({"type": "Sample", "child": TRUE}, "The field 'size' is required in a Sample expression"),
    (dict(OK, size=-1), SIZE),
    (dict(OK, size="3"), SIZE),
    (dict(OK, size=2.5), SIZE),
    (dict(OK, size=None), SIZE),
    (dict(OK, size=2 ** 31), SIZE),
    (dict(OK, size=2 ** 63), SIZE),
    (dict(OK, seed=-1), SEED),
    (dict(OK, seed="7"), SEED),
    (dict(OK, seed=1.5), SEED),
    (dict(OK, seed=None), SEED),
    (dict(OK, seed=2 ** 63), SEED),
    (dict(OK, seed=2 ** 64), SEED),
    (dict(OK, dateField="date"), TOGETHER),
    (dict(OK, dateRanges=[WEEK]), TOGETHER),
    (_strata(WEEK, dateField=5), "The field 'dateField' in a Sample expression needs to be a string"),
    (dict(OK, dateField="date", dateRanges=WEEK), RANGES),
    (dict(OK, dateField="date", dateRanges="2021"), RANGES),
    (_strata(WEEK, "2021-01-11"), RANGES),
    (_strata(WEEK, [NEXT_WEEK]), RANGES),
    (_strata(*[{"dateFrom": f"{2000 + k // 12}-{k % 12 + 1:02d}-01", "dateTo": f"{2000 + k // 12}-{k % 12 + 1:02d}-02"} for k in range(1025)]),
     "A Sample expression takes at most 1024 date ranges"),
    (_strata({"dateFrom": 20210104}), "The field 'dateFrom' of a date range in a Sample expression needs to be a string or null"),
    (_strata({"dateTo": True}), "The field 'dateTo' of a date range in a Sample expression needs to be a string or null"),
    (_strata({"dateFrom": "2021-13-01"}), "The dateFrom '2021-13-01' of a date range in a Sample expression is not a valid date (YYYY-MM-DD)"),
    (_strata({"dateTo": "yesterday"}), "The dateTo 'yesterday' of a date range in a Sample expression is not a valid date (YYYY-MM-DD)"),
    (_strata({"dateFrom": "2021-01-10", "dateTo": "2021-01-04"}),
     "A date range in a Sample expression has dateFrom after dateTo: " + json.dumps({"dateFrom": "2021-01-10", "dateTo": "2021-01-04"}, separators=(",", ":"))),
    (_strata(WEEK, {"dateFrom": "2021-01-10", "dateTo": "2021-01-12"}), OVERLAP),  # both ends are inclusive: one shared day overlaps
    (_strata(WEEK, WEEK), OVERLAP),
    (_strata({"dateTo": "2021-01-04"}, WEEK), OVERLAP),
    (_strata(WEEK, {}), OVERLAP),
    ({"type": "And", "children": [TRUE, dict(OK, size=-1)]}, SIZE),
    ({"type": "Not", "child": {"type": "Maybe", "child": dict(OK, seed=-1)}}, SEED),
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
