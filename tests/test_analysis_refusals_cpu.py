"""CPU-only: the stand-alone analysis entries of the C ABI refuse what tests/golden/analysis_refusals.json recorded
(tools/dump_analysis_refusals.py, run at the commit the file names in ``generated_at``): per case the return code and the WHOLE text
of ``mi_last_error()``, per workspace query the size.  Every pointer is a fixed fake address and every recorded call is refused
before anything is read through one.  Nothing here may be skipped: a case that cannot be replayed fails."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_spec = importlib.util.spec_from_file_location("dump_analysis_refusals", os.path.join(ROOT, "tools", "dump_analysis_refusals.py"))
refusals = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(refusals)

with open(os.path.join(ROOT, "tests", "golden", "analysis_refusals.json")) as _f:
    GOLDEN = json.load(_f)


def test_the_record_is_whole():
    """The cases are the tool's, in its order; every entry has every documented rule of its list broken alone and together with all
    later ones; every recorded call was refused with MI_EINVAL and a message; every query is there with a size."""
    tool = [json.loads(json.dumps(list(c))) for c in refusals.cases()]
    assert [row[:4] for row in GOLDEN["cases"]] == tool and len(tool) > 250
    assert len(refusals.ENTRIES) == 7 and len(refusals.QUERIES) == 4
    for name, entry in refusals.ENTRIES.items():
        assert len(entry["rules"]) >= 5, name
        for label, _ in entry["rules"]:
            for how in ("alone", "with later"):
                assert sum(row[:3] == [name, label, how] for row in GOLDEN["cases"]) == 1, (name, label, how)
        # "with later" breaks more than "alone".  (Which rule then speaks is held by the recorded message, replayed whole below; the
        # rule lists are the tool's reading of include/midd.h and are not parsed from it.)
        for label, _ in entry["rules"][:-1]:
            alone, later = ([row for row in GOLDEN["cases"] if row[:3] == [name, label, how]][0] for how in ("alone", "with later"))
            assert len(later[3]) > len(alone[3]), (name, label)
    assert all(row[4] == -1 and row[5] for row in GOLDEN["cases"])
    queries = [[name, list(args)] for name, table in refusals.QUERIES.items() for args in table]
    assert [row[:2] for row in GOLDEN["queries"]] == queries
    for name in refusals.QUERIES:
        sizes = [row[2] for row in GOLDEN["queries"] if row[0] == name]
        assert sum(s > 0 for s in sizes) >= 4 and sum(s == 0 for s in sizes) >= 4, name
    assert all((row[2] == 0) == (row[3] is not None) for row in GOLDEN["queries"])
    assert len(GOLDEN["generated_at"]) == 40, "recorded at a clean commit"


def test_every_recorded_refusal_is_given_again():
    native = refusals.load()
    wrong = []
    for name, label, how, changes, rc, message in GOLDEN["cases"]:
        got = refusals.call(native, name, changes)
        if got != (rc, message):
            wrong.append((name, label, how, changes, [rc, message], got))
    assert not wrong, f"{len(wrong)} refusals changed; the first: {wrong[:3]}"


def test_every_recorded_query_answers_the_same():
    native = refusals.load()
    wrong = []
    for name, args, size, message in GOLDEN["queries"]:
        got = refusals.query(native, name, args)
        if got != (size, message):
            wrong.append((name, args, [size, message], got))
    assert not wrong, f"{len(wrong)} answers changed; the first: {wrong[:3]}"
