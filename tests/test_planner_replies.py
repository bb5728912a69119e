"""Every planner.* reply of tests/planner_script.py on the host-only planner
(no engine, no GPU) against tests/golden/planner_replies_cpu.json, exactly.
The recording was taken from the commit before the planner methods were put on
one request front, so it pins what that change must not move: the five placing
methods answer "planner: no engine bound" only after the front, the sync and
their own checks have run; assume, forget, encode, sync and every error answer
in full; engineCalls counts the engine-less calls."""
import json

import planner_script as S


def test_replies_equal_the_recording():
    want = S.load("planner_replies_cpu.json")
    got = json.loads(json.dumps(S.run(None)))
    assert [e[0] for e in got] == [e[0] for e in want]
    for g, w in zip(got, want):
        assert g == w, g[0]
    # the recording itself: the errors the issue quotes, and the accounting
    err = {label: e for label, _, e in want}
    assert err["plan"] == err["explain"] == err["gangs"] == err["fit lowest"] == err["bind plan"] == "planner: no engine bound"
    assert err["no planner: planner.plan"] == "no placement planner bound to this cache"
    assert err["65 classes: planner.plan"] == "placement planner: more than 64 requirement classes"
    assert err["span not a level"].endswith("is not one of the engine's topology levels")
    assert "is finer than the topology key" in err["span finer than key"]
    assert err["fit no policy"].startswith("planner.planFit: policy (none) is none of ")
    assert err["bind assignment a number"].startswith("planner.bind: assignment must be a plan or an object")
    assert err["assume assignment a list"].startswith("planner.assume: assignment must be a plan or an object")
    res = {label: r for label, r, _ in want}
    assert (res["assume plan"]["committed"], res["assume plan"]["stale"]) == (3, 1)
    assert res["forget"]["forgotten"] == ["train-w-1"]
    # 15 placing calls without an engine; the span errors, assume and forget count nothing
    assert res["engineCalls"] == 15 and res["engineCalls without a planner"] == 0
