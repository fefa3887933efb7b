"""The texts of the 400 responses for malformed positionFrom / positionTo of a CellCount filter expression and for malformed
CellCountByRegion actions, byte for byte, and the toString of a CellCount with and without a region: without the two fields it is
what it was before they existed.  tests/host_tools/filter_strings_main.cpp (one request per line through the JSON parser and the
Expression and Action builders; the filter's toString or the message per line) is linked against the built engine library, without
sanitizers, and run as its own process.  Parsing needs no GPU.  The messages that need a database — a region past the end of the
sequence, a sharded database — are compared, byte for byte as well, by tests/test_region_cell_count_gpu.py with PAST_THE_END,
REGION_PAST_THE_END and SHARDED below."""
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
REGION = {"name": "a", "positionFrom": 1, "positionTo": 10}
ACTION = {"type": "CellCountByRegion", "cells": "missing", "atMost": 0, "regions": [REGION]}
POSITION = "The field '{}' in a CellCount expression, if present, needs to be an integer from 1 to 4294967295"
FROM, TO = POSITION.format("positionFrom"), POSITION.format("positionTo")
ORDER = "The field 'positionFrom' in a CellCount expression may not be greater than 'positionTo'"
PAST_THE_END = "CellCount: the field positionTo: {} is past the end of the sequence '{}' ({} positions)"
FROM_PAST_THE_END = "CellCount: the field positionFrom: {} is past the end of the sequence '{}' ({} positions)"
REGION_PAST_THE_END = "CellCountByRegion: the region '{}': positionTo {} is past the end of the sequence '{}' ({} positions)"
SHARDED = {
    "CellCount": "CellCount is not supported on a sharded database yet: the table of cell counts of a position shard is partial",
    "CellCountByRegion": "CellCountByRegion is not supported on a sharded database yet: its counts are not all-reduced across ranks",
}
BEFORE = "The default nucleotide sequence has between 0 and 3000 cells that are missing"  # CellCount::toString as K22 wrote it
KINDS = "one of \"substitutions\", \"deletions\", \"missing\", \"ambiguous\" or a non-empty list of them without repeats"
A = "CellCountByRegion action: "
REGIONS = A + "the field regions must be an array of 1 to 256 objects"
NO_REGIONS = A + "the field regions is required"
REGION_NAME = A + "every region must have the field name of type string"
TWICE = A + "the region 'a' is listed more than once: the names of the regions must be distinct"
REGION_POSITION = A + "the region 'a': the field {} must be an integer from 1 to 2147483647"
REGION_NO_POSITION = A + "the region 'a': the field {} is required"
REGION_ORDER = A + "the region 'a': the field positionFrom may not be greater than positionTo"
REGION_BOUND = A + "the region 'a': the field {}, if present, must be an integer from 0 to 4294967295"
ACTION_BOUND = A + "the field {}, if present, must be an integer from 0 to 4294967295"
UNBOUNDED = A + "the region '{}' has no bound: at least one of the fields atLeast and atMost is required, in the region or in the action"

EXPRESSION_CASES = [
    (OK, BEFORE),
    (dict(OK, sequenceName="S", cells=["substitutions", "missing"], atLeast=2), "The sequence 'S' has between 2 and 3000 cells that are substitutions+missing"),
    ({"type": "CellCount", "cells": "deletions", "atLeast": 9}, "The default nucleotide sequence has between 9 and 4294967295 cells that are deletions"),
    (dict(OK, positionFrom=21563, positionTo=25384), BEFORE + " in the positions 21563 to 25384"),
    (dict(OK, positionFrom=7), BEFORE + " in the positions 7 to the end"),
    (dict(OK, positionTo=7), BEFORE + " in the positions 1 to 7"),
    (dict(OK, positionFrom=7, positionTo=7), BEFORE + " in the positions 7 to 7"),
    (dict(OK, positionFrom=1, positionTo=4294967295), BEFORE + " in the positions 1 to 4294967295"),  # (a database knows the length)
    ({"type": "Not", "child": dict(OK, positionTo=3)}, "!(" + BEFORE + " in the positions 1 to 3)"),
    (dict(OK, positionFrom=0), FROM),
    (dict(OK, positionFrom=-1), FROM),
    (dict(OK, positionFrom=1.5), FROM),
    (dict(OK, positionFrom="1"), FROM),
    (dict(OK, positionFrom=None), FROM),
    (dict(OK, positionFrom=[1]), FROM),
    (dict(OK, positionFrom=True), FROM),
    (dict(OK, positionFrom=4294967296), FROM),
    (dict(OK, positionTo=0), TO),
    (dict(OK, positionTo=-5), TO),
    (dict(OK, positionTo=2.5), TO),
    (dict(OK, positionTo="9"), TO),
    (dict(OK, positionTo=None), TO),
    (dict(OK, positionTo={"to": 3}), TO),
    (dict(OK, positionTo=4294967296), TO),
    (dict(OK, positionFrom=0, positionTo=0), FROM),
    (dict(OK, positionFrom=8, positionTo=7), ORDER),
    (dict(OK, positionFrom=4294967295, positionTo=1), ORDER),
    ({"type": "And", "children": [TRUE, dict(OK, positionFrom=3, positionTo=2)]}, ORDER),
]

ACTION_CASES = [
    (ACTION, "ok"),
    (dict(ACTION, sequenceName="S", cells=["missing", "ambiguous"], atLeast=1), "ok"),
    ({"type": "CellCountByRegion", "cells": "missing", "regions": [dict(REGION, atLeast=3)]}, "ok"),
    ({"type": "CellCountByRegion", "cells": "missing", "regions": [dict(REGION, atMost=0), dict(REGION, name="b", atLeast=1, atMost=2)]}, "ok"),
    (dict(ACTION, regions=[dict(REGION, name=str(g)) for g in range(256)]), "ok"),
    (dict(ACTION, regions=[REGION, dict(REGION, name="b", positionFrom=5, positionTo=2147483647)]), "ok"),  # overlapping; a database knows the length
    (dict(ACTION, orderByFields=["region", "positionFrom", "positionTo", {"field": "count", "order": "descending"}], limit=3, offset=1), "ok"),
    ({"type": "CellCountByRegion", "cells": "missing", "atMost": 0}, NO_REGIONS),
    (dict(ACTION, regions=[]), REGIONS),
    (dict(ACTION, regions=REGION), REGIONS),
    (dict(ACTION, regions="a"), REGIONS),
    (dict(ACTION, regions=None), REGIONS),
    (dict(ACTION, regions=[REGION, "b"]), REGIONS),
    (dict(ACTION, regions=[[REGION]]), REGIONS),
    (dict(ACTION, regions=[dict(REGION, name=str(g)) for g in range(257)]), REGIONS),
    (dict(ACTION, regions=[{"positionFrom": 1, "positionTo": 3}]), REGION_NAME),
    (dict(ACTION, regions=[dict(REGION, name=3)]), REGION_NAME),
    (dict(ACTION, regions=[dict(REGION, name=None)]), REGION_NAME),
    (dict(ACTION, regions=[REGION, dict(REGION, name="b"), dict(REGION, positionFrom=20, positionTo=30)]), TWICE),
    (dict(ACTION, regions=[{"name": "a", "positionTo": 3}]), REGION_NO_POSITION.format("positionFrom")),
    (dict(ACTION, regions=[{"name": "a", "positionFrom": 3}]), REGION_NO_POSITION.format("positionTo")),
    (dict(ACTION, regions=[dict(REGION, positionFrom=0)]), REGION_POSITION.format("positionFrom")),
    (dict(ACTION, regions=[dict(REGION, positionFrom="1")]), REGION_POSITION.format("positionFrom")),
    (dict(ACTION, regions=[dict(REGION, positionFrom=1.5)]), REGION_POSITION.format("positionFrom")),
    (dict(ACTION, regions=[dict(REGION, positionTo=0)]), REGION_POSITION.format("positionTo")),
    (dict(ACTION, regions=[dict(REGION, positionTo=None)]), REGION_POSITION.format("positionTo")),
    (dict(ACTION, regions=[dict(REGION, positionTo=2147483648)]), REGION_POSITION.format("positionTo")),
    (dict(ACTION, regions=[dict(REGION, positionFrom=11)]), REGION_ORDER),
    (dict(ACTION, regions=[dict(REGION, atLeast=-1)]), REGION_BOUND.format("atLeast")),
    (dict(ACTION, regions=[dict(REGION, atLeast="2")]), REGION_BOUND.format("atLeast")),
    (dict(ACTION, regions=[dict(REGION, atMost=4294967296)]), REGION_BOUND.format("atMost")),
    (dict(ACTION, regions=[dict(REGION, atMost=None)]), REGION_BOUND.format("atMost")),
    (dict(ACTION, atLeast=-1), ACTION_BOUND.format("atLeast")),
    (dict(ACTION, atMost=1.5), ACTION_BOUND.format("atMost")),
    (dict(ACTION, atMost=4294967296), ACTION_BOUND.format("atMost")),
    ({"type": "CellCountByRegion", "cells": "missing", "regions": [REGION]}, UNBOUNDED.format("a")),
    ({"type": "CellCountByRegion", "cells": "missing", "regions": [dict(REGION, atMost=1), dict(REGION, name="second")]}, UNBOUNDED.format("second")),
    ({"type": "CellCountByRegion", "atMost": 0, "regions": [REGION]}, A + "the field cells is required"),
    (dict(ACTION, cells="none"), A + "the field cells must be " + KINDS),
    (dict(ACTION, cells=[]), A + "the field cells must be " + KINDS),
    (dict(ACTION, sequenceName=3), A + "the field sequenceName, if present, must be of type string"),
]


def test_parse_messages_and_strings(built, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    program = str(tmp_path / "filter_strings")
    build = subprocess.run(
        ["g++", "-O1", "-std=c++20", "-I", os.path.join(ROOT, "include"), "-I", HOST, os.path.join(ROOT, "tests", "host_tools", "filter_strings_main.cpp"),
         "-o", program, "-L", LIB, "-lsilo_engine", "-lsilo_gpu", "-Wl,-rpath," + LIB, "-Wl,-rpath-link," + LIB, "-pthread"],
        capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    cases = [({"action": {"type": "Aggregated"}, "filterExpression": expression}, want) for expression, want in EXPRESSION_CASES]
    cases += [({"action": action, "filterExpression": TRUE}, "True" if want == "ok" else want) for action, want in ACTION_CASES]
    requests = "".join(json.dumps(request) + "\n" for request, _ in cases)
    run = subprocess.run([program], input=requests.encode(), capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr.decode(errors="replace")[-3000:]
    got = run.stdout.decode().split("\n")
    assert got[-1] == "" and len(got) == len(cases) + 1
    for (request, want), message in zip(cases, got):
        assert message == want, request
