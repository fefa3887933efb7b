"""The texts of the 400 responses for malformed CellCount filter expressions and CellCountDistribution actions, byte for byte.  The
program of tests/test_action_parse_messages.py (tests/host_tools/parse_messages_main.cpp: one request per line through the JSON parser
and the Expression and Action builders, `ok` or the message per line) is linked here against the built engine library, without
sanitizers, and run as its own process.  Parsing needs no GPU.  The messages for a sequence the database does not have, for a sharded
database and for a field the action cannot order by come from a database: tests/test_cell_count_gpu.py compares them, byte for byte as
well, with UNKNOWN_SEQUENCE and SHARDED below."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "lapis-silo_amd", "host")
LIB = os.path.join(ROOT, "lapis-silo_amd", "lib")
TRUE = {"type": "True"}
OK = {"type": "CellCount", "cells": "missing", "atMost": 3000}
ACTION = {"type": "CellCountDistribution", "cells": "missing"}
KINDS = "one of \"substitutions\", \"deletions\", \"missing\", \"ambiguous\" or a non-empty list of them without repeats"
CELLS = "The field 'cells' in a CellCount expression needs to be " + KINDS
NAME = "The field 'sequenceName' in a CellCount expression, if present, needs to be a string"
NO_CELLS = "The field 'cells' is required in a CellCount expression"
NO_BOUND = "At least one of the fields 'atLeast' and 'atMost' is required in a CellCount expression"
AT_LEAST = "The field 'atLeast' in a CellCount expression, if present, needs to be an integer from 0 to 4294967295"
AT_MOST = "The field 'atMost' in a CellCount expression, if present, needs to be an integer from 0 to 4294967295"
ACTION_CELLS = "CellCountDistribution action: the field cells must be " + KINDS
ACTION_NO_CELLS = "CellCountDistribution action: the field cells is required"
ACTION_NAME = "CellCountDistribution action: the field sequenceName, if present, must be of type string"
BIN_WIDTH = "CellCountDistribution action: the field binWidth, if present, must be an integer of at least 1"
MAX_BINS = "CellCountDistribution action: the field maxBins, if present, must be an integer from 1 to 4096"
PRODUCT = ("CellCountDistribution action: the fields binWidth and maxBins: their product must not exceed 2147483648, so that every bin's bounds are "
           "32-bit numbers")
UNKNOWN_SEQUENCE = "{}: the field sequenceName: Database does not contain a sequence with name: '{}'"
SHARDED = {
    "CellCount": "CellCount is not supported on a sharded database yet: the table of cell counts of a position shard is partial",
    "CellCountDistribution": "CellCountDistribution is not supported on a sharded database yet: its counts are not all-reduced across ranks",
}

EXPRESSION_CASES = [
    (OK, "ok"),
    (dict(OK, sequenceName="S"), "ok"),
    (dict(OK, sequenceName="no such sequence"), "ok"),  # (known only to a database)
    (dict(OK, cells=["missing"]), "ok"),
    (dict(OK, cells=["ambiguous", "missing", "deletions", "substitutions"]), "ok"),
    ({"type": "CellCount", "cells": "substitutions", "atLeast": 60}, "ok"),
    ({"type": "CellCount", "cells": "deletions", "atLeast": 9, "atMost": 8}, "ok"),  # legal: selects nothing
    ({"type": "CellCount", "cells": "deletions", "atLeast": 0, "atMost": 4294967295}, "ok"),
    ({"type": "Not", "child": OK}, "ok"),
    ({"type": "DistinctSequences", "child": {"type": "Sample", "child": OK, "size": 3}}, "ok"),
    ({"type": "CellCount", "atMost": 3}, NO_CELLS),
    ({"type": "CellCount"}, NO_CELLS),
    (dict(OK, cells="Missing"), CELLS),
    (dict(OK, cells="insertions"), CELLS),
    (dict(OK, cells=""), CELLS),
    (dict(OK, cells=[]), CELLS),
    (dict(OK, cells=["missing", "missing"]), CELLS),
    (dict(OK, cells=["missing", "ambiguous", "missing"]), CELLS),
    (dict(OK, cells=["missing", 3]), CELLS),
    (dict(OK, cells=[["missing"]]), CELLS),
    (dict(OK, cells=3), CELLS),
    (dict(OK, cells=None), CELLS),
    (dict(OK, cells={"kind": "missing"}), CELLS),
    (dict(OK, sequenceName=5), NAME),
    (dict(OK, sequenceName=None), NAME),
    (dict(OK, sequenceName=["S"]), NAME),
    ({"type": "CellCount", "cells": "missing"}, NO_BOUND),
    ({"type": "CellCount", "cells": "missing", "atleast": 3}, NO_BOUND),
    (dict(OK, atMost=-1), AT_MOST),
    (dict(OK, atMost=1.5), AT_MOST),
    (dict(OK, atMost="3"), AT_MOST),
    (dict(OK, atMost=None), AT_MOST),
    (dict(OK, atMost=4294967296), AT_MOST),
    (dict(OK, atMost=[3]), AT_MOST),
    (dict(OK, atLeast=-1), AT_LEAST),
    (dict(OK, atLeast=0.5), AT_LEAST),
    (dict(OK, atLeast="0"), AT_LEAST),
    (dict(OK, atLeast=None), AT_LEAST),
    (dict(OK, atLeast=4294967296), AT_LEAST),
    (dict(OK, atLeast=True), AT_LEAST),
    ({"type": "And", "children": [TRUE, {"type": "CellCount", "cells": "missing"}]}, NO_BOUND),
    ({"type": "Not", "child": {"type": "Maybe", "child": dict(OK, cells="x")}}, CELLS),
]

ACTION_CASES = [
    (ACTION, "ok"),
    (dict(ACTION, cells=["missing", "ambiguous"], sequenceName="S", binWidth=100, maxBins=4096), "ok"),
    (dict(ACTION, binWidth=2147483647, maxBins=1), "ok"),
    (dict(ACTION, binWidth=524288, maxBins=4096), "ok"),
    (dict(ACTION, orderByFields=["from", {"field": "count", "order": "descending"}], limit=3, offset=1), "ok"),
    ({"type": "CellCountDistribution"}, ACTION_NO_CELLS),
    ({"type": "CellCountDistribution", "binWidth": 2}, ACTION_NO_CELLS),
    (dict(ACTION, cells="none"), ACTION_CELLS),
    (dict(ACTION, cells=[]), ACTION_CELLS),
    (dict(ACTION, cells=["deletions", "deletions"]), ACTION_CELLS),
    (dict(ACTION, cells=7), ACTION_CELLS),
    (dict(ACTION, cells=None), ACTION_CELLS),
    (dict(ACTION, sequenceName=3), ACTION_NAME),
    (dict(ACTION, sequenceName=["main"]), ACTION_NAME),
    (dict(ACTION, binWidth=0), BIN_WIDTH),
    (dict(ACTION, binWidth=-2), BIN_WIDTH),
    (dict(ACTION, binWidth=1.5), BIN_WIDTH),
    (dict(ACTION, binWidth="2"), BIN_WIDTH),
    (dict(ACTION, binWidth=None), BIN_WIDTH),
    (dict(ACTION, binWidth=2147483648), BIN_WIDTH),
    (dict(ACTION, maxBins=0), MAX_BINS),
    (dict(ACTION, maxBins=4097), MAX_BINS),
    (dict(ACTION, maxBins=-1), MAX_BINS),
    (dict(ACTION, maxBins=2.0), MAX_BINS),
    (dict(ACTION, maxBins="8"), MAX_BINS),
    (dict(ACTION, maxBins=None), MAX_BINS),
    (dict(ACTION, binWidth=2147483647, maxBins=2), PRODUCT),
    (dict(ACTION, binWidth=2097153), PRODUCT),  # times the default of 1 024 bins
    (dict(ACTION, binWidth=524289, maxBins=4096), PRODUCT),
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
    cases = [({"action": {"type": "Aggregated"}, "filterExpression": expression}, want) for expression, want in EXPRESSION_CASES]
    cases += [({"action": action, "filterExpression": TRUE}, want) for action, want in ACTION_CASES]
    requests = "".join(json.dumps(request) + "\n" for request, _ in cases)
    run = subprocess.run([program], input=requests.encode(), capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr.decode(errors="replace")[-3000:]
    got = run.stdout.decode().split("\n")
    assert got[-1] == "" and len(got) == len(cases) + 1
    for (request, want), message in zip(cases, got):
        assert message == want, request
