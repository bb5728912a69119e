"""One engine driven through tests/call_sequences.py's seeded scripts: patches
of every size, assume / forget, re-uploads, service mode changes and idle gaps
with every placement and planner call in between, every reply and the metrics
totals compared with the host model. A failure names the seed, the world, the
op and the mutating ops since the last reply that matched;

    python tests/call_sequences.py --seed S --world W --upto K

replays that prefix alone. The last test of each world asserts that the paths
the world is there for did answer: the compaction service and the lease in
`compact`, the split service in `split`, the host walk and a GPU walker in
`launch`, the shard combine in `set`."""
import collections
import time

import pytest

import call_sequences as cs

pytestmark = pytest.mark.gpu

SEEN = {w: {} for w in cs.WORLDS}     # world -> seed -> (who answered per op, seconds)


@pytest.fixture
def single(engine):
    yield engine
    engine.service_stop()
    engine.set_service(True)          # the default mode
    engine.set_fused(True)
    engine.set_timing(False)


@pytest.fixture(scope="module")
def device_set():
    from jobset_amd.engine import Engine
    e = Engine(devices=[0, 0, 0])
    yield e
    e.close()


def run(engine, world, seed):
    p, ops = cs.script(seed, world)
    replies, totals = cs.expected(p, ops), cs.expected_totals(p, ops)   # all before the first engine call
    cs.setup(engine, world)
    t0 = time.perf_counter()
    who = cs.replay(engine, p, ops, replies, totals, seed=seed, world=world)
    SEEN[world][seed] = (who, time.perf_counter() - t0)


def seen(world):
    """What the world's cases recorded. Nothing runs here: a case that did not
    complete has failed by itself, and its script is not replayed."""
    missing = sorted(set(cs.SEEDS[world]) - set(SEEN[world]))
    assert not missing, f"the sequence cases of world {world} did not complete: seeds {missing}"
    shapes = collections.Counter()
    leased = 0
    for who, _ in SEEN[world].values():
        for kind, fused, lease in who:
            if fused is not None:
                shapes[(kind, fused)] += 1
            leased += lease
    slow = max((dt, seed) for seed, (_, dt) in SEEN[world].items())
    print(f"{world}: shapes {dict(sorted(shapes.items()))}, lease answers {leased}, "
          f"slowest script seed {slow[1]} {slow[0]:.2f} s")
    return {f for (kind, f) in shapes if kind == "place"}, {f for (_, f) in shapes}, leased


@pytest.mark.parametrize("world,seed", [(w, s) for w in cs.WORLDS for s in cs.SEEDS[w]], ids=lambda v: str(v))
def test_sequence(request, world, seed):
    run(request.getfixturevalue("device_set" if world == "set" else "single"), world, seed)


def test_launch_world_took_both_walks():
    placed, shapes, _ = seen("launch")
    assert 7 in shapes and shapes & {0, 1, 2}, shapes
    # jsp_place itself: a GPU walker for the batches; the repeated batch (256 jobs and more, classes on several
    # levels) is walked on the host, behind the launch path's own tally (7) or the split tiles' (8)
    assert placed & {0, 1, 2} and placed & {7, 8}, placed
    assert not placed & {3, 5}, placed                    # the service is off in this world


def test_split_world_met_the_split_service():
    placed, _, _ = seen("split")
    assert 5 in placed, placed


def test_compact_world_met_the_service_and_the_lease():
    placed, _, leased = seen("compact")
    assert 3 in placed, placed
    assert leased > 0


def test_device_set_world_combined_the_shards():
    placed, _, _ = seen("set")
    assert placed == {6}, placed
