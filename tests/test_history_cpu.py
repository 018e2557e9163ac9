"""The catalogue of the call-history tests (tests/history_cases.py) checked without a device: every expectation is computable from the
CPU restatements and deterministic; every excursion can show in some action's expectation (otherwise it could leave nothing behind that
a successor would reveal); and every symbol the library exports is reached by the catalogue or is on the short NOT_IN_MATRIX list."""
import importlib

import pytest

import history_cases as HC

ALLOWED_REASONS = ("lifecycle", "profiling", "pure host function", "ingest")


@pytest.fixture(scope="module")
def world():
    return HC.make_world()


@pytest.mark.one_arith
def test_catalogue_sizes():
    assert HC.SIZES == dict(actions=43, action_forms=77, excursions=25, refusals=9), HC.SIZES
    assert len(HC.predecessors()) == 77 + 25 + 9
    for e in HC.EXCURSIONS:
        assert e.work and all(n in HC.BY_NAME for n in e.work), e.name


def test_every_expectation_is_computable_and_deterministic(world, arith):
    st = HC.state(arith)
    firsts = [a.expected(world, st) for a in HC.ACTIONS]
    again = HC.make_world()   # nothing cached: the detections tracking_ref and tracking_orb_ref remember per image are dropped too
    HC.TR._detected.clear()
    HC.TOR._detected.clear()
    HC.TOR._walked.clear()
    for a, first in zip(HC.ACTIONS, firsts):
        second = a.expected(again, st)
        assert first and all(isinstance(v, bytes) for v in first.values()), a.name
        assert first.keys() == second.keys() and HC.first_difference(second, first) is None, (a.name, HC.first_difference(second, first))
    # the baseline itself is not degenerate: every pair of every pose call succeeds, every table and every match list has rows
    for a in HC.ACTIONS:
        want = a.expected(world, st)
        for k, v in want.items():
            if k.endswith(".status"):
                assert v == b"\0\0\0\0" and k.replace(".status", ".pose") in want, (a.name, k)
            assert len(v) > 0 or k.startswith(("absent",)), (a.name, k)


def test_every_excursion_governs_an_action(world, arith):
    """Discrimination: under the state an excursion's work runs in, at least one action's expectation differs from its baseline
    expectation in at least one byte — and one of the excursion's own work actions is among them, so the work that is compared under the
    excursion is work a leak would change."""
    base = HC.state(arith)
    table = []
    for e in HC.EXCURSIONS:
        alt = e.state(arith)
        changed = {k for k in alt if alt[k] != base[k]}
        assert changed, e.name
        candidates = [a for a in HC.ACTIONS if "arith" in changed or changed & set(a.reads)]
        governs = [a.name for a in candidates if HC.first_difference(a.expected(world, alt), a.expected(world, base)) is not None]
        table.append((e.name, sorted(changed), governs))
        assert governs, "excursion %s changes no expectation: give it other inputs" % e.name
        assert set(governs) & set(e.work), (e.name, governs, e.work)
    width = max(len(n) for n, _, _ in table)
    print("\nexcursion -> the actions it governs (%s)" % arith)
    for name, changed, governs in table:
        print("  %-*s  %-22s  %s" % (width, name, ",".join(changed), " ".join(governs)))


@pytest.mark.one_arith
def test_every_export_is_in_the_matrix_or_excused():
    capi = importlib.import_module("uw-slam_amd.capi")
    exports, reached = set(capi.SYMBOLS), HC.reached()
    assert reached <= exports, sorted(reached - exports)
    assert not reached & set(HC.NOT_IN_MATRIX), sorted(reached & set(HC.NOT_IN_MATRIX))
    assert set(HC.NOT_IN_MATRIX) <= exports, sorted(set(HC.NOT_IN_MATRIX) - exports)
    for name, reason in HC.NOT_IN_MATRIX.items():
        assert reason in ALLOWED_REASONS, (name, reason)
    missing = sorted(exports - reached - set(HC.NOT_IN_MATRIX))
    assert not missing, "exports in neither group (add an action to tests/history_cases.py): %s" % missing
    assert len(HC.NOT_IN_MATRIX) <= 25
    print("\nreached: %d exports; NOT_IN_MATRIX: %d" % (len(reached), len(HC.NOT_IN_MATRIX)))
