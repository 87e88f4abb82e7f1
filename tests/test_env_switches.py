"""The RP_* environment variables the package reads are exactly those in INTEGRATION.md's table: a switch that the code
reads but the table does not name is a fork nobody can find, and one the table names but nothing reads is a dead promise.
Names only (os.environ in rec_pangu_amd/**/*.py, getenv in rec_pangu_amd/csrc/*): no kernel is looked at."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rec_pangu_amd")

# one read = the accessor immediately followed by the variable's name as a string literal
PY_READ = re.compile(r"""os\.environ(?:\.get|\.setdefault|\.pop)?\s*[(\[]\s*["'](\w+)["']""")
C_READ = re.compile(r"""\bgetenv\s*\(\s*"(\w+)"\s*\)""")


def _reads(pattern, accessor, paths):
    """{name: first place it is read}; every use of the accessor must name its variable literally, so that none can hide
    behind an alias (env = os.environ.get) or a computed name"""
    found = {}
    for path in sorted(paths):
        with open(path, encoding="utf-8") as f:
            text = f.read()
        names = pattern.findall(text)
        uses = len(re.findall(accessor, text))
        where = os.path.relpath(path, ROOT)
        assert uses == len(names), f"{where}: {uses} uses of {accessor} but {len(names)} name their variable literally"
        for n in names:
            found.setdefault(n, where)
    return found


def _read_by_the_package():
    py = _reads(PY_READ, r"os\.environ\b", glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True))
    c = _reads(C_READ, r"\bgetenv\b", [p for p in glob.glob(os.path.join(PKG, "csrc", "*")) if os.path.isfile(p)])
    return {n: w for n, w in {**c, **py}.items() if n.startswith("RP_")}


def _documented():
    """the first column of the table whose header row starts with | Name |"""
    with open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8") as f:
        lines = f.read().splitlines()
    start = [i for i, l in enumerate(lines) if re.match(r"\|\s*Name\s*\|", l)]
    assert len(start) == 1, "INTEGRATION.md must hold exactly one table of environment variables (| Name | ... |)"
    names = []
    for l in lines[start[0] + 2:]:
        if not l.startswith("|"):
            break
        cell = l.split("|")[1].strip()
        m = re.fullmatch(r"`(RP_[A-Z0-9_]+)`", cell)
        assert m, f"INTEGRATION.md: the first cell of a row is one variable name in backticks, not {cell!r}"
        names.append(m.group(1))
    assert len(set(names)) == len(names), "INTEGRATION.md: a variable is listed twice"
    return set(names)


def test_environment_switches_match_the_documented_table():
    read, doc = _read_by_the_package(), _documented()
    assert read and doc
    undocumented = sorted(f"{n} (read in {read[n]})" for n in set(read) - doc)
    unread = sorted(doc - set(read))
    assert not undocumented, "read by the package but missing from INTEGRATION.md's table: " + ", ".join(undocumented)
    assert not unread, "in INTEGRATION.md's table but read nowhere in the package: " + ", ".join(unread)
