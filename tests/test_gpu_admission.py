"""Every entry point on every kind of handle answers what tests/golden/admission_matrix.json recorded (admission_cases.py):
the same cells, the same return codes, a message for every refusal, and a refused call leaves the handle as it was."""
from __future__ import annotations

import json
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import admission_cases as ac  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matrix(golden_dir):
    return json.loads((golden_dir / "admission_matrix.json").read_text())


def test_fixture_covers_every_state(matrix):
    assert len(matrix["recorded_at"]) == 40
    assert sorted(matrix["cells"]) == sorted(ac.STATES)


@pytest.mark.parametrize("state", list(ac.STATES))
def test_admission(vdb, matrix, state):
    report = {}
    got = ac.run_state(vdb, state, report)
    want = matrix["cells"][state]
    assert sorted(got) == sorted(want)                          # no cell skipped, none left out of the fixture
    assert len(got) == len(ac.entries(ac.ctx(ac.STATES[state].d, ac.STATES[state].n, ac.STATES[state].byte_valued)))
    differ = {e: (got[e], want[e]) for e in got if got[e] != want[e]}
    assert not differ, f"(got, recorded): {differ}"
    assert not report["no_message"], report["no_message"]
    assert not report["changed"], report["changed"]
