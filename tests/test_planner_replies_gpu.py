"""Every planner.* reply of tests/planner_script.py with the engine bound,
against tests/golden/planner_replies_gpu.json, exactly: the recording was taken
on an MI355X from the commit before the planner methods were put on one request
front. One test, about 70 host calls on a 16-node cluster. The floors below are
asserted on the recording itself, so a degenerate one cannot hide a failure."""
import json

import pytest

import planner_script as S

pytestmark = pytest.mark.gpu


def uploads(x, into):
    """Every "upload" value anywhere in a reply."""
    if isinstance(x, dict):
        for k, v in x.items():
            if k == "upload":
                into.add(v)
            uploads(v, into)
    elif isinstance(x, list):
        for v in x:
            uploads(v, into)
    return into


def check_floors(entries):
    res = {label: r for label, r, _ in entries}
    err = {label: e for label, _, e in entries}
    for label in ("plan", "plan previous", "explain", "gangs", "fit tightest", "bind plan", "assume plan",
                  "plan after assume", "recreate previousPlan"):
        assert err[label] is None, (label, err[label])
    assert any(j["domain"] is None for j in res["plan"]["jobs"]) and res["plan"]["placed"] >= 1
    sticky = res["plan previous"]
    assert min(sticky["kept"], sticky["moved"], sticky["lost"]) >= 1
    assert res["explain"]["explanations"]
    gangs = [g for label in res if label.startswith("gangs") for g in res[label]["jobSets"]]
    assert any(not g["placed"] for g in gangs)
    assert any(g["placed"] and g["spanKey"] is not None and g["spanDomain"] is not None for g in gangs)
    assert any(j["topologyKey"] == "zone" and j["domain"] is not None
               for label in res if label.startswith("gangs") for j in res[label]["jobs"])
    fits = {tuple(j["domainId"] for j in res["fit " + p]["jobs"]) for p in S.POLICIES}
    assert len(fits) >= 2
    assert any(res[b]["stale"] >= 1 and res[b]["bound"] >= 1 for b in ("bind plan", "bind map", "bind unknown value"))
    assert res["assume plan"]["committed"] >= 1 and res["assume plan"]["stale"] >= 1
    assert res["plan after assume"]["snapshot"]["upload"] == "patch"
    assert res["sync after class errors"]["upload"] == "patch"      # the class errors before it synced nothing
    assert {"full", "patch", "none"} <= uploads([r for _, r, _ in entries], set())


def test_replies_equal_the_recording(engine):
    want = S.load("planner_replies_gpu.json")
    check_floors(want)
    got = json.loads(json.dumps(S.run(engine)))
    assert [e[0] for e in got] == [e[0] for e in want]
    for g, w in zip(got, want):
        assert g == w, g[0]
