"""The call-sequence machinery of tests/sequence_cases.py, proven on the host: the generator is deterministic and its
committed seed sets meet every coverage condition, the driver passes on the fake indexes over every committed sequence (a few hundred
rows, the same steps), every planted stale-state fault is caught by a committed sequence at or after the first step where it can show,
and `replay` rebuilds the failing prefix.  No GPU and no broken library: the faults live in the NumPy fakes."""
from __future__ import annotations

import pytest

from tests import sequence_cases as sc

KINDS = ("flat", "ivf")
CASES = [(kind, shape.name, seed) for kind in KINDS for shape, seed in sc.committed(kind)]


def _run_fake(oracle, kind, name, seed, fault=None, steps=None):
    shape = sc.shape_of(kind, name).reduced()
    metric = sc.metric_of(shape, seed)
    steps = sc.sequence(kind, name, seed) if steps is None else steps
    sc.run(sc.open_fake(shape, metric, fault), steps, sc.model_for(shape, metric, oracle), label=f"{kind} {name} seed {seed} {metric}")


def test_generator_is_deterministic():
    first = {c: sc.sequence(*c) for c in CASES}
    sc._chain.cache_clear()
    assert all(sc.sequence(*c) == first[c] for c in CASES)
    assert all(len(steps) == sc.STEPS for steps in first.values())
    assert sc.sequence("flat", "dense", 99) == sc.sequence("flat", "dense", 99)          # (a seed outside the committed set)
    assert sc.replay("ivf", "f16-d64", 2, 11) == first[("ivf", "f16-d64", 2)][:12]


@pytest.mark.parametrize("kind", KINDS)
def test_committed_seeds_cover_every_ordered_pair_and_every_probe_after_every_dropper(kind):
    cov = sc.Coverage.empty(kind)
    for shape, seed in sc.committed(kind):
        steps = sc.sequence(kind, shape.name, seed)
        _, installed, ranged = sc.dry_run(shape, sc.metric_of(shape, seed), steps)
        cov.add(kind, steps, installed, ranged)
    feasible = sc.feasible_pairs(kind)
    missing = sorted(feasible - cov.pairs)
    assert not missing, f"{len(missing)} ordered pairs never occur: {missing}\n" + sc.pair_matrix(kind, cov.pairs)
    assert cov.pairs <= feasible, sorted(cov.pairs - feasible)                              # (the rule of what can follow what holds)
    # an infeasible pair is one the preconditions rule out, not one the generator avoids: few, and for the stated reasons only
    assert len(feasible) >= len(sc.OPS[kind]) ** 2 - {"flat": 14 + 13 + 1, "ivf": 2 * 12 + 3 * 11}[kind]
    unprobed = {d: sorted(set(sc.PROBES) - seen) for d, seen in cov.probes.items() if set(sc.PROBES) - seen}
    assert not unprobed, unprobed


@pytest.mark.parametrize("kind,name,seed", CASES, ids=[f"{k}-{n}-s{s}" for k, n, s in CASES])
def test_every_sequence_repeats_a_batch_size_and_regrows_under_a_filter(kind, name, seed):
    shape = sc.shape_of(kind, name)
    steps = sc.sequence(kind, name, seed)
    answers, installed, _ = sc.dry_run(shape, sc.metric_of(shape, seed), steps)
    lines = "\n".join(s.line() for s in steps)
    assert sc.same_size_pair(steps, answers) is not None, lines
    assert sc.regrowth_step(steps, answers, installed) is not None, lines
    assert sum(1 for s, a in zip(steps, answers) if s.op == "search" and not a) <= 1, lines       # (one search of an empty index at most)


@pytest.mark.parametrize("kind,name,seed", CASES, ids=[f"{k}-{n}-s{s}" for k, n, s in CASES])
def test_driver_passes_on_the_unfaulted_fake(kind, name, seed, oracle):
    _run_fake(oracle, kind, name, seed)


@pytest.mark.parametrize("fault,kind", [(f, k) for f, kinds in sc.FAULTS.items() for k in kinds],
                         ids=[f"{f}-{k}" for f, kinds in sc.FAULTS.items() for k in kinds])
def test_every_planted_fault_is_caught(fault, kind, oracle):
    caught = None
    for shape, seed in sc.committed(kind):
        steps = sc.sequence(kind, shape.name, seed)
        trigger = sc.fault_trigger(fault, shape, sc.metric_of(shape, seed), steps)
        if trigger is None:
            continue
        try:
            _run_fake(oracle, kind, shape.name, seed, fault)
        except sc.SequenceMismatch as e:
            assert e.step >= trigger, (fault, shape.name, seed, e.step, trigger)
            assert f"step {e.step} " in str(e) and f"seed {seed}" in str(e) and str(e).count("\n") == e.step + 1     # (the whole trace)
            caught = (shape.name, seed, e.step)
            break
    assert caught is not None, f"no committed {kind} sequence catches '{fault}'"
    print(f"{fault} on {kind}: caught by {caught[0]} seed {caught[1]} at step {caught[2]}")
    # the prefix that `replay` rebuilds fails at the same step, and one step less passes
    name, seed, step = caught
    with pytest.raises(sc.SequenceMismatch) as again:
        _run_fake(oracle, kind, name, seed, fault, sc.replay(kind, name, seed, step))
    assert again.value.step == step
    _run_fake(oracle, kind, name, seed, fault, sc.replay(kind, name, seed, step - 1))


def test_trace_file_names_the_step_before_it_runs(tmp_path, monkeypatch, oracle):
    path = tmp_path / "trace.txt"
    monkeypatch.setenv("VDBHIP_SEQUENCE_TRACE", str(path))
    kind, name, seed = "flat", "dense", 0
    steps = sc.sequence(kind, name, seed)
    trigger = sc.fault_trigger("refused-add-changes-ntotal", sc.shape_of(kind, name), "l2", steps)
    if trigger is None:
        _run_fake(oracle, kind, name, seed)
        assert len(path.read_text().splitlines()) == len(steps)
        return
    with pytest.raises(sc.SequenceMismatch) as e:
        _run_fake(oracle, kind, name, seed, "refused-add-changes-ntotal")
    lines = path.read_text().splitlines()
    assert len(lines) == e.value.step + 1 and lines[-1].endswith(steps[e.value.step].line())
