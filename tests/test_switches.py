"""The run-time switch table of DESIGN.md ("Run-time switches") is the list of TSPLAT_* environment
variables the package reads: no more, no fewer, and every name a test or bench.py sets is on it
(or is read only outside the package)."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "transplat_amd"
NAME = r"(TSPLAT_[A-Z0-9_]+)"
# os.environ.get("X") / os.environ["X"] / os.getenv("X") / "X" in os.environ; getenv("X") in C
PY_READ = re.compile(r"os\.(?:environ(?:\.\w+)?\s*[\[(]|getenv\()\s*[\"']" + NAME + r"[\"']|[\"']" + NAME
                     + r"[\"']\s+(?:not\s+)?in\s+os\.environ")
C_READ = re.compile(r"getenv\(\s*\"" + NAME + r"\"")
# what a test or bench.py sets: monkeypatch.setenv / delenv, os.environ[...] =, env dict literals
# (TSPLAT_X=..., {"TSPLAT_X": ...}) and tuples of knob names -- every quoted or keyword name
SET = re.compile(r"[\"']" + NAME + r"[\"']|\b" + NAME + r"=")
READ_OUTSIDE_PACKAGE = {"TSPLAT_DIST_BACKEND"}  # bench.py's process-group backend


def _names(pattern, files):
    found = set()
    for f in files:
        for m in pattern.finditer(f.read_text()):
            found.update(g for g in m.groups() if g)
    return found


def package_reads():
    py = _names(PY_READ, sorted(PKG.rglob("*.py")))
    c = _names(C_READ, sorted(p for p in (PKG / "csrc").iterdir() if p.is_file()))
    return py | c


def table_names():
    text = (ROOT / "DESIGN.md").read_text()
    start = text.index("Run-time switches\n")
    section = text[start:text.index("\n## ", start)]
    return {m.group(1) for m in re.finditer(r"^\| `" + NAME + r"` \|", section, re.M)}


def test_table_lists_what_the_package_reads():
    reads, table = package_reads(), table_names()
    print(f"{len(reads)} names read by the package, {len(table)} rows in the table")
    assert reads - table == set(), "read by the package, missing from DESIGN.md's table"
    assert table - reads == set(), "in DESIGN.md's table, read nowhere in the package"


def test_names_set_by_tests_and_bench_are_in_the_table():
    files = sorted(p for p in (ROOT / "tests").rglob("*.py") if p.name != Path(__file__).name) + [ROOT / "bench.py"]
    used = _names(SET, files)
    assert READ_OUTSIDE_PACKAGE & package_reads() == set()
    assert used - table_names() - READ_OUTSIDE_PACKAGE == set()
