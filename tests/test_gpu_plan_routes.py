"""The plan's dispatch (csrc/plan.hip: which kernel runs each conv slot in each direction, which launches walk a need or
flat-field list) against tests/golden/plan_launches.json, recorded by tools/record_plan_launches.py on the commit named
in the file: for every case and call, the ordered (family, VGG module) list of ``profile_launches()`` and the SHA-256 of
the results' bytes are the recorded ones.  The cases and the calls are the recorder's own (one definition); only the
fixture is read."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_plan_launches", os.path.join(ROOT, "tools", "record_plan_launches.py"))
REC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(REC)

with open(os.path.join(ROOT, "tests", "golden", "plan_launches.json")) as _f:
    GOLDEN = json.load(_f)


def test_fixture_holds_every_case_and_the_listed_launches():
    assert len(GOLDEN["recorded_at_commit"]) == 40
    assert sorted(GOLDEN["cases"]) == sorted(REC.case_name(*c) for c in REC.CASES)
    assert not [n for n in GOLDEN["nondeterministic"] if "=" not in n], "a default-environment case without hashes"
    for name in ("B2_S64", "B1_S128"):
        fams = {f for c in GOLDEN["cases"][name]["calls"].values() for f, _ in GOLDEN["launch_lists"][c["launches"]]}
        assert {"conv43_dgrad_need", "convx_dgrad_need", "conv43_fwd_flat", "flat_fill"} <= fams, (name, sorted(fams))


@pytest.mark.parametrize("B,S,env", REC.CASES, ids=[REC.case_name(*c) for c in REC.CASES])
def test_plan_launches_and_results_are_the_recorded_ones(monkeypatch, B, S, env):
    for k in REC.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)            # before the handle is made: it reads its switches then
    name = REC.case_name(B, S, env)
    want = GOLDEN["cases"][name]
    assert (want["B"], want["S"], want["env"]) == (B, S, env)
    got = REC.run_case(B, S)
    assert sorted(got) == sorted(want["calls"])
    hashed = name not in GOLDEN["nondeterministic"]
    for call, rec in want["calls"].items():
        assert got[call]["launches"] == GOLDEN["launch_lists"][rec["launches"]], (name, call, "launch list differs")
        if hashed:
            assert got[call]["sha256"] == rec["sha256"], (name, call, "result bytes differ")
