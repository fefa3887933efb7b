"""The texts of the 400 responses for malformed MeanDistances / AminoAcidMeanDistances actions, byte for byte.
tests/host_tools/filter_strings_main.cpp (one request per line through the JSON parser and the Expression and Action builders; the
filter's toString or the message per line) is linked against the built engine library, without sanitizers, and run as its own
process.  Parsing needs no GPU.  The messages that need a database — a region past the end of the sequence, a sharded database — are
compared, byte for byte as well, by tests/test_mean_distances_gpu.py."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "lapis-silo_amd", "host")
LIB = os.path.join(ROOT, "lapis-silo_amd", "lib")
TRUE = {"type": "True"}
GROUP = {"name": "a", "filterExpression": TRUE}
REGION = {"name": "r", "positionFrom": 1, "positionTo": 10}
ACTION = {"type": "MeanDistances", "groups": [GROUP], "regions": [REGION]}
AMINO = dict(ACTION, type="AminoAcidMeanDistances", sequenceName="S")
A = "MeanDistances action: "
ENTRY = "{\"name\": string, \"filterExpression\": filter expression}"
GROUPS = A + "the field groups, if present, must be an array of objects " + ENTRY
GROUP_OBJECT = A + "every entry of groups must be an object " + ENTRY
GROUP_NAME = A + "every entry of groups must contain the field name of type string"
GROUP_FILTER = A + "the field filterExpression of the group '{}' must be of type object (a filter expression)"
REGIONS = A + "the field regions, if present, must be an array of 1 to 256 objects"
REGION_NAME = A + "every region must have the field name of type string"
TWICE = A + "the region 'r' is listed more than once: the names of the regions must be distinct"
REGION_POSITION = A + "the region 'r': the field {} must be an integer from 1 to 2147483647"
REGION_NO_POSITION = A + "the region 'r': the field {} is required"
REGION_ORDER = A + "the region 'r': the field positionFrom may not be greater than positionTo"
ROW_CAP = A + "{} regions x {} {} are {} rows, more than the 65536 a response may hold"


def _groups(n):
    return [dict(GROUP, name=str(g)) for g in range(n)]


def _regions(n):
    return [dict(REGION, name=str(r)) for r in range(n)]


CASES = [
    (ACTION, "ok"),
    ({"type": "MeanDistances"}, "ok"),
    (AMINO, "ok"),
    ({"type": "AminoAcidMeanDistances", "sequenceName": "S"}, "ok"),
    (dict(ACTION, sequenceName="main", between=False, orderByFields=["region", {"field": "meanDistance", "order": "descending"}], limit=3, offset=1), "ok"),
    (dict(ACTION, groups=_groups(64), regions=_regions(31)), "ok"),  # 31 x 2 080 = 64 480 rows
    (dict(ACTION, groups=_groups(64), regions=_regions(256), between=False), "ok"),  # 256 x 64 = 16 384
    (dict(ACTION, groups=_groups(22), regions=_regions(256)), "ok"),  # 256 x 253 = 64 768
    (dict(ACTION, regions=[REGION, dict(REGION, name="b", positionFrom=5, positionTo=2147483647)]), "ok"),  # overlapping; a database knows the length
    (dict(ACTION, groups=_groups(64), regions=_regions(32)), ROW_CAP.format(32, 2080, "pairs of groups", 66560)),
    (dict(ACTION, groups=_groups(23), regions=_regions(256)), ROW_CAP.format(256, 276, "pairs of groups", 70656)),
    (dict(ACTION, groups=_groups(23), regions=_regions(256), between=True), ROW_CAP.format(256, 276, "pairs of groups", 70656)),
    (dict(ACTION, sequenceName=3), A + "the field sequenceName, if present, must be of type string"),
    (dict(ACTION, sequenceName=["main"]), A + "the field sequenceName, if present, must be of type string"),
    ({"type": "AminoAcidMeanDistances"}, "AminoAcidMeanDistances action must contain the field sequenceName of type string (a gene)"),
    (dict(AMINO, sequenceName=None), "AminoAcidMeanDistances action: the field sequenceName, if present, must be of type string"),
    (dict(ACTION, groups=GROUP), GROUPS),
    (dict(ACTION, groups="a"), GROUPS),
    (dict(ACTION, groups=None), GROUPS),
    (dict(ACTION, groups=[]), A + "the field groups, if present, must hold at least one group"),
    (dict(ACTION, groups=_groups(65)), A + "the field groups holds 65 groups, more than the limit of 64"),
    (dict(ACTION, groups=[GROUP, 5]), GROUP_OBJECT),
    (dict(ACTION, groups=[[GROUP]]), GROUP_OBJECT),
    (dict(ACTION, groups=[{"filterExpression": TRUE}]), GROUP_NAME),
    (dict(ACTION, groups=[GROUP, {"name": 5, "filterExpression": TRUE}]), GROUP_NAME),
    (dict(ACTION, groups=[GROUP, dict(GROUP)]), A + "the name 'a' occurs more than once in groups"),
    (dict(ACTION, groups=[{"name": "b"}]), GROUP_FILTER.format("b")),
    (dict(ACTION, groups=[GROUP, {"name": "b", "filterExpression": "True"}]), GROUP_FILTER.format("b")),
    (dict(ACTION, groups=[{"name": "c", "filterExpression": {"type": "NoSuchFilter"}}]),
     A + "the field filterExpression of the group 'c' is not a valid filter expression: Unknown object filter type 'NoSuchFilter'"),
    (dict(ACTION, regions=[]), REGIONS),
    (dict(ACTION, regions=REGION), REGIONS),
    (dict(ACTION, regions="r"), REGIONS),
    (dict(ACTION, regions=None), REGIONS),
    (dict(ACTION, regions=[REGION, "b"]), REGIONS),
    (dict(ACTION, regions=[[REGION]]), REGIONS),
    (dict(ACTION, regions=_regions(257)), REGIONS),
    (dict(ACTION, regions=[{"positionFrom": 1, "positionTo": 3}]), REGION_NAME),
    (dict(ACTION, regions=[dict(REGION, name=3)]), REGION_NAME),
    (dict(ACTION, regions=[dict(REGION, name=None)]), REGION_NAME),
    (dict(ACTION, regions=[REGION, dict(REGION, name="b"), dict(REGION, positionFrom=20, positionTo=30)]), TWICE),
    (dict(ACTION, regions=[{"name": "r", "positionTo": 3}]), REGION_NO_POSITION.format("positionFrom")),
    (dict(ACTION, regions=[{"name": "r", "positionFrom": 3}]), REGION_NO_POSITION.format("positionTo")),
    (dict(ACTION, regions=[dict(REGION, positionFrom=0)]), REGION_POSITION.format("positionFrom")),
    (dict(ACTION, regions=[dict(REGION, positionFrom="1")]), REGION_POSITION.format("positionFrom")),
    (dict(ACTION, regions=[dict(REGION, positionFrom=1.5)]), REGION_POSITION.format("positionFrom")),
    (dict(ACTION, regions=[dict(REGION, positionFrom=-1)]), REGION_POSITION.format("positionFrom")),
    (dict(ACTION, regions=[dict(REGION, positionTo=0)]), REGION_POSITION.format("positionTo")),
    (dict(ACTION, regions=[dict(REGION, positionTo=None)]), REGION_POSITION.format("positionTo")),
    (dict(ACTION, regions=[dict(REGION, positionTo=True)]), REGION_POSITION.format("positionTo")),
    (dict(ACTION, regions=[dict(REGION, positionTo=2147483648)]), REGION_POSITION.format("positionTo")),
    (dict(ACTION, regions=[dict(REGION, positionFrom=11)]), REGION_ORDER),
    (dict(AMINO, regions=[dict(REGION, positionFrom=11)]), "AminoAcid" + REGION_ORDER),
    (dict(ACTION, between="true"), A + "the field between, if present, must be of type boolean"),
    (dict(ACTION, between=1), A + "the field between, if present, must be of type boolean"),
    (dict(ACTION, between=None), A + "the field between, if present, must be of type boolean"),
    ({"type": "MeanDistance"}, "MeanDistance is not a valid action"),
]


def test_parse_messages(built, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    program = str(tmp_path / "filter_strings")
    build = subprocess.run(
        ["g++", "-O1", "-std=c++20", "-I", os.path.join(ROOT, "include"), "-I", HOST, os.path.join(ROOT, "tests", "host_tools", "filter_strings_main.cpp"),
         "-o", program, "-L", LIB, "-lsilo_engine", "-lsilo_gpu", "-Wl,-rpath," + LIB, "-Wl,-rpath-link," + LIB, "-pthread"],
        capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    requests = "".join(json.dumps({"action": action, "filterExpression": TRUE}) + "\n" for action, _ in CASES)
    run = subprocess.run([program], input=requests.encode(), capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr.decode(errors="replace")[-3000:]
    got = run.stdout.decode().split("\n")
    assert got[-1] == "" and len(got) == len(CASES) + 1
    for (action, want), message in zip(CASES, got):
        assert message == ("True" if want == "ok" else want), action
