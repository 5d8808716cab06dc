"""What a plan allocates (st3d_plan_bytes) against tests/golden/plan_decisions.json: for every recorded row with S <= 128 and
B <= 4 -- sizes times switches, the switches of the handle included -- the plan made under the row's environment holds
exactly the recorded number of bytes.  The rows were recorded on the commit before the plan's lists came to be allocated
by one function for the batch and for each group, so the test holds that function to what the separate blocks allocated:
no list more, none less, none of another size."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_plan_launches", os.path.join(ROOT, "tools", "record_plan_launches.py"))
REC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(REC)

with open(os.path.join(ROOT, "tests", "golden", "plan_decisions.json")) as _f:
    _DOC = json.load(_f)
ROWS = [dict(r, **{"in": _DOC["inputs"][r["in"]]}) for r in _DOC["rows"]]       # (each distinct input is stored once)
ROWS = [r for r in ROWS if r["in"]["S"] <= 128 and r["in"]["B"] <= 4]
SIZES = sorted({(r["in"]["B"], r["in"]["S"]) for r in ROWS})
# every switch a row may set: the handle's (read when the handle is made) and the plan's (read by st3d_plan_create)
HANDLE = ("ST3D_CONV", "ST3D_WINO43", "ST3D_WINO43_MINK", "ST3D_PREGATE", "ST3D_TAP0_FUSED")
SWITCHES = HANDLE + ("ST3D_NEED_FORCE", "ST3D_KEEP_FORCE", "ST3D_NEED_TILE", "ST3D_KEEP_TILE", "ST3D_KEEP_SHALLOW", "ST3D_NEED_DEPTH",
                     "ST3D_FLAT_DEPTH", "ST3D_KEEP_DEPTH", "ST3D_NEED_BLOCKS", "ST3D_NEED_GRAM", "ST3D_SPLIT_BATCH", "ST3D_FLAT_CONV1")


def test_the_rows_cover_the_sizes_and_every_switch():
    assert SIZES == [(B, S) for B in (1, 2, 4) for S in (64, 128)] and len(ROWS) == 6 * 38
    assert {k for r in ROWS for k in r["env"]} == set(SWITCHES) - {"ST3D_FLAT_CONV1"}
    assert len({r["bytes"] for r in ROWS}) > 40          # the switches do move the figure


@pytest.mark.parametrize("B,S", SIZES, ids=["B%d_S%d" % s for s in SIZES])
def test_plan_bytes_are_the_recorded_ones(monkeypatch, B, S):
    from st3d import vgg as V
    dev = torch.device("cuda:0")
    nets = {}
    bad = []
    for row in (r for r in ROWS if (r["in"]["B"], r["in"]["S"]) == (B, S)):
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in row["env"].items():
            monkeypatch.setenv(k, v)
        handle = tuple(sorted((k, v) for k, v in row["env"].items() if k in HANDLE))
        if handle not in nets:          # the handle reads its switches when it is made
            nets[handle] = V.Vgg19Features(REC._state(), device=dev)
        plan = V.PerceptualPlan(nets[handle], B, S)
        try:
            if plan.bytes() != row["bytes"]:
                bad.append((row["env"], plan.bytes(), row["bytes"]))
        finally:
            plan.close()
    assert not bad, bad
