"""The scripts of tests/call_sequences.py on the references alone (no GPU):
that a seed gives one script, that every expected reply passes the checkers
the per-call suites use, and that the committed seeds can expose something --
every kind often enough, every reading kind directly behind every mutating
and every planner kind, and enough replies that differ from what the same
call would get on the snapshot the script started from, which is what makes a
stale table, a held-back patch or a stale lease visible."""
import collections
import functools

import numpy as np
import pytest

from oracle import oracle as O

import call_sequences as cs
import whatif_ref
from bind_ref import check_bind
from gang_ref import check_gangs
from preempt_ref import check_preempt
from spread_ref import check_spread
from sticky_ref import check_sticky

CASES = [(w, s) for w in cs.WORLDS for s in cs.SEEDS[w]]


@functools.lru_cache(maxsize=None)
def scripted(world, seed):
    p, ops = cs.script(seed, world)
    return p, ops, cs.expected(p, ops), cs.expected_totals(p, ops)


def kinds_of(world):
    read = cs.SET_READ if world == "set" else cs.READ
    mut = ("patch", "classes", "reupload") if world == "set" else cs.MUTATING
    return read, mut


def test_seed_lists():
    for w in cs.WORLDS:
        assert len(cs.SEEDS[w]) == 12 and len(set(cs.SEEDS[w])) == 12
        # one script per rotation of the deck
        assert sorted(s % cs.ROTATIONS for s in cs.SEEDS[w]) == list(range(12)), w
    assert all(cs.split_shape(s) for s in cs.SEEDS["split"])
    for s in cs.SEEDS["compact"]:
        p = cs.world_problem(s, "compact")[0]
        assert len(p.classes) == 1 and p.classes[0].level == p.topology.n_levels - 1


@pytest.mark.parametrize("world,seed", CASES)
def test_deterministic(world, seed):
    p, ops, replies, totals = scripted(world, seed)
    p2, ops2 = cs.script(seed, world)
    replies2, totals2 = cs.expected(p2, ops2), cs.expected_totals(p2, ops2)
    assert len(ops) == len(ops2) and all(cs.same(a, b) for a, b in zip(ops, ops2))
    assert all(cs.same(a, b) for a, b in zip(replies, replies2)) and totals == totals2


@pytest.mark.parametrize("world,seed", CASES)
def test_length_and_last_stop(world, seed):
    _, ops, _, _ = scripted(world, seed)
    assert 30 <= len(ops) <= 48, len(ops)
    assert ops[-1]["kind"] == "service" and ops[-1]["mode"] == "stop"
    assert sum(op["kind"] == "sleep" for op in ops) <= 2
    # parked mode never meets the device path: a stop and a mode change come first
    parked = False
    for op in ops:
        if op["kind"] == "service":
            parked = op["mode"] == "parked" or (parked and op["mode"] == "stop")
        assert not (parked and op["kind"] == "place_device")
    for op in ops:
        if op["kind"] == "patch":
            assert np.unique(op["rows"]).shape == op["rows"].shape      # distinct rows
            assert any(op[c] is not None for c in ("labels", "taints", "free", "excl"))


@pytest.mark.parametrize("world,seed", CASES)
def test_replies_pass_the_checkers(world, seed):
    """Every expected reply, on the model's snapshot at its step."""
    p, ops, replies, _ = scripted(world, seed)
    m = cs.Model(p, [], [])
    for i, (op, r) in enumerate(zip(ops, replies)):
        got = m.apply(op)
        assert cs.same(got, r), i
        k = op["kind"]
        if k not in cs.READ:
            continue
        q = m.view(op["jobs"]) if "jobs" in op else m.p
        tl = O.place_c(q)[1:] if "jobs" in op else None
        if k in ("place", "place_device"):
            O.check_invariants(q, r["assign"], *tl)
        elif k == "sticky":
            check_sticky(q, op["prev"], r["assign"], tl)
            kept = (r["assign"] == op["prev"]) & (op["prev"] >= 0)
            assert r["stats"]["kept"] <= int(kept.sum())
        elif k == "gangs":
            check_gangs(q, op["gang_jobs"], op["gang_span"], r["assign"], r["span"], tl)
        elif k == "fit":
            check_sticky(q, None, r["assign"], tl)          # I1 / I2 of any answer
        elif k == "spread":
            check_spread(q, op["level"], op["max_skew"], op["peers"], r["assign"], r["spread"], r["count"], tl)
        elif k == "preempt":
            check_preempt(q, op["prio"], op["owners"], op["ranks"], op["evict_free"], r["assign"], r["victim_off"],
                          r["victims"])
        elif k == "whatif":
            for s, sc in enumerate(op["scenarios"]):
                qs = whatif_ref.patched(q, sc)
                O.check_invariants(qs, r["assign"][s], *O.place_c(qs)[1:])
        elif k == "bind":
            bound, pods = check_bind(q, op["assign"], r["pod_row"], r["pod_off"])
            assert (bound, pods) == (r["stats"]["bound"], r["stats"]["pods_bound"])
        elif k == "explain":
            for rec in r["records"]:
                assert rec["rows"] == rec["rows_selector"] + rec["rows_taint"] + rec["rows_no_capacity"] + rec["rows_fit"]
                assert rec["domains"] == rec["dom_occupied"] + rec["dom_short"] + rec["dom_feasible"]


def test_row_domain_against_a_row_table():
    """row_domain (searchsorted) against a table built row by row."""
    for seed in range(12):
        p = cs.world_problem(seed, "launch")[0]
        N, K = p.nodes.n_nodes, p.topology.n_levels
        leaf = p.nodes.leaf_of_row()
        rows = np.concatenate([np.arange(-2, N + 2), [-(1 << 31), (1 << 31) - 1]])
        for k in range(K + 2):
            want = np.full(rows.shape, -1, dtype=np.int64)
            if k < K:
                parent = p.topology.parent_of_leaf(k)
                ok = (rows >= 0) & (rows < N)
                want[ok] = parent[leaf[rows[ok]]]
            np.testing.assert_array_equal(cs.row_domain(p, rows, np.full(rows.shape, k)), want)
        np.testing.assert_array_equal(cs.row_domain(p, [0], [0xFFFFFFFF]), [-1])


# ---------------------------------------------------------------- coverage over the committed seeds
@pytest.mark.parametrize("world", cs.WORLDS)
def test_every_kind_often_enough(world):
    read, mut = kinds_of(world)
    kinds, sizes = collections.Counter(), collections.Counter()
    for s in cs.SEEDS[world]:
        for op in scripted(world, s)[1]:
            kinds[op["kind"]] += 1
            if op["kind"] == "patch":
                sizes[op["size"]] += 1
    for k in read + mut + ("refusal", "service"):
        assert kinds[k] >= 6, (world, k, kinds[k])
    for z in cs.SIZES:
        assert sizes[z] >= 6, (world, z, sizes[z])


@pytest.mark.parametrize("world", cs.WORLDS)
def test_every_column_subset_and_place_variant(world):
    """All 15 non-empty subsets of a patch's four columns, jsp_place in each of
    its forms, and a refusal of every call family the world has."""
    masks, variants, families = collections.Counter(), collections.Counter(), set()
    for s in cs.SEEDS[world]:
        for op in scripted(world, s)[1]:
            if op["kind"] == "patch":
                cols = sum(b for b, c in ((1, "labels"), (2, "taints"), (4, "free"), (8, "excl")) if op[c] is not None)
                assert cols == op["mask"]
                masks[cols] += 1
            elif op["kind"] == "place":
                variants[op["variant"]] += 1
            elif op["kind"] == "refusal":
                families.add(op["family"])
    assert sorted(masks) == list(range(1, 16)) and min(masks.values()) >= 4, (world, masks)
    assert set(variants) == set(cs.PLACE_VARIANTS) and min(variants.values()) >= 3, (world, variants)
    want = cs.PLANNER + ("place", "patch") + (() if world == "set" else ("assume", "forget"))
    assert families == set(want), (world, families)


@pytest.mark.parametrize("world", ("launch", "split", "compact"))
def test_the_patterns_that_expose_stale_state(world):
    """What a stale claim table, a lease a forget did not give up, or a fit
    that skips a held-back patch would show in, counted on the model: it must
    be there in most scripts, not in one."""
    forgets = lease = fits = stickies = 0
    for s in cs.SEEDS[world]:
        _, ops, replies, _ = scripted(world, s)
        kinds = [op["kind"] for op in ops]
        f = kinds.index("forget")
        assert kinds.count("forget") == 1 and kinds[f - 1] == "place" and "assume" in kinds[f - 4:f]
        assert not any(op["kind"] == "reupload" or (op["kind"] == "patch" and op["excl"] is not None)
                       for op in ops[kinds.index("assume"):f])
        forgets += replies[f]["cleared"] > 0
        # the placement two calls behind the forget differs from the one in front of it: a lease kept shows
        after = next(i for i in range(f + 2, len(ops)) if kinds[i] == "place" and ops[i]["variant"] == "all")
        assert after == f + 2
        lease += not cs.same(replies[f - 1]["assign"], replies[after]["assign"])
        # place, a one-row patch, fit: the fit's reply differs from what it would be without the patch
        i = next(i for i, op in enumerate(ops) if op["kind"] == "patch" and op["size"] == "one")
        assert kinds[i - 1] == "place" and kinds[i + 1] == "fit"
        m = cs.Model(scripted(world, s)[0], [], [])
        for op in ops[:i]:
            m.apply(op)
        fits += not cs.same(m.apply(ops[i + 1]), replies[i + 1])
        stickies += sum(k in ("sticky", "bind") for k in kinds) >= 3
    assert forgets >= 10, (world, forgets)
    assert lease >= 6, (world, lease)
    assert fits >= 6, (world, fits)
    assert stickies >= 6, (world, stickies)


@pytest.mark.parametrize("world", cs.WORLDS)
def test_every_reader_directly_behind_every_writer_and_planner(world):
    read, mut = kinds_of(world)
    pairs = set()
    for s in cs.SEEDS[world]:
        ops = scripted(world, s)[1]
        pairs |= {(a["kind"], b["kind"]) for a, b in zip(ops, ops[1:])}
    for y in read:
        for x in ("patch", "assume", "forget"):
            if x in mut:
                assert (x, y) in pairs, (world, x, y)
        for x in cs.PLANNER:
            if x in read and x != y:
                assert (x, y) in pairs, (world, x, y)


def _partial(op, r):
    """The reply places at least one job and leaves at least one (explain:
    feasible and infeasible domains both)."""
    if op["kind"] == "explain":
        return any(rec["dom_feasible"] > 0 and rec["dom_feasible"] < rec["domains"] for rec in r["records"])
    if op["kind"] == "bind":
        return 0 < r["stats"]["bound"] < r["stats"]["jobs"]
    a = np.asarray(r["assign"])
    return bool((a >= 0).any() and (a < 0).any())


@pytest.mark.parametrize("world", cs.WORLDS)
def test_replies_depend_on_the_state(world):
    """Of the ops that read rows, a third at least get another reply than on
    the script's initial snapshot, and half at least are neither empty nor full."""
    n = moved = partial = 0
    for s in cs.SEEDS[world]:
        p, ops, replies, _ = scripted(world, s)
        for op, r in zip(ops, replies):
            if op["kind"] not in cs.ROW_READERS:
                continue
            fresh = cs.Model(p, [], []).apply(op)
            n += 1
            moved += not cs.same(fresh, r)
            partial += _partial(op, r)
    assert 3 * moved >= n, (world, moved, n)
    assert 2 * partial >= n, (world, partial, n)
