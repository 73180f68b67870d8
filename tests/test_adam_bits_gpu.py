"""The fused Adam against ``tests/golden/adam_bits.json``, bit for bit: every step form (``step``,
``graphable``, ``graphable`` with the counter advanced by hand, ``pack``) with every combination
of clipping, schedule and weight average, a skipped update per form and a priming launch
(``tests/adam_bits.py`` holds the cases and the runner).

The golden file was recorded by ``tests/adam_bits.py --record`` from the commit it names, the one
before ``optim.hip``'s update rule, prologue and launchers were unified, and is never recorded
from the code under test.  After a compiler upgrade it may be re-recorded from an unchanged
``optim.hip``; re-recording it from a changed one is not a fix: a mismatch then means the change
altered the arithmetic."""
import json
import os

import pytest

import adam_bits

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(__file__), "golden", "adam_bits.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(autouse=True)
def _no_switch(monkeypatch):
    for k in adam_bits.SWITCHES:
        monkeypatch.delenv(k, raising=False)


def test_golden_covers_the_cases():
    assert sorted(GOLDEN["cases"]) == sorted(adam_bits.cases()) and len(GOLDEN["cases"]) == 37
    assert GOLDEN["commit"] and "clang version" in GOLDEN["hipcc"]


@pytest.mark.parametrize("name", sorted(adam_bits.cases()))
def test_bits_match_the_record(name):
    got, want = adam_bits.run_case(name), GOLDEN["cases"][name]
    assert sorted(got) == sorted(want), name
    wrong = [k for k in want if got[k] != want[k]]
    assert not wrong, f"{name}: {wrong} differ from the record of {GOLDEN['commit'][:12]}"
