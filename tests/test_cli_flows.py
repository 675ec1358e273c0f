"""What the hdr2yuv program prints, returns and writes on the runs of tests/golden/make_cli_flows.py, against the record of them in
tests/golden/cli_flows.json: the exit status, every stdout line and the md5 of every written file of every run.  The record was
taken from the program when each of its five flows still had a loop of its own; the one loop that drives them all now (run_block,
hdr2yuv_amd/cli/hdr2yuv.cpp) has to do the same."""
import importlib.util
import json
import os

import pytest

import h2y_testing as ht

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_cli_flows", os.path.join(ROOT, "tests", "golden", "make_cli_flows.py"))
flows = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(flows)

with open(flows.GOLDEN) as _f:
    GOLDEN = json.load(_f)


def test_every_case_is_recorded():
    assert sorted(GOLDEN) == sorted(flows.CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(flows.CASES))
def test_cli_flow(name):
    got, want = flows.record(ht.exe(), name), GOLDEN[name]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g["stdout"] == w["stdout"], (name, k)
        assert g["status"] == w["status"], (name, k)
        assert g["wrote"] == w["wrote"], (name, k)
