"""Every measurement the docs cite exists: the `profiles/...` records and the
`tools/...` scripts named in DESIGN.md, README.md, INTEGRATION.md and
tools/README.md (a record split over a line break is matched by its prefix;
`{a,b}` alternatives and `*` globs are expanded)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOCS = ("DESIGN.md", "README.md", "INTEGRATION.md", "tools/README.md")


def _refs(kind):
    out = []
    for doc in DOCS:
        text = open(os.path.join(ROOT, doc)).read()
        for m in re.finditer(kind + r"/([A-Za-z0-9_.*{},\-]+)", text):
            ref = m.group(1).rstrip(".,;:)")
            if not ref:
                continue
            alts = [ref]
            mm = re.match(r"(.*)\{([^}]*)\}(.*)", ref)
            if mm:
                alts = [mm.group(1) + a + mm.group(3) for a in mm.group(2).split(",")]
            out += [(doc, a) for a in alts if "{" not in a]
    return out


def test_cited_profiles_exist():
    missing = [(d, p) for d, p in _refs("profiles")
               if not glob.glob(os.path.join(ROOT, "profiles", p)) and not glob.glob(os.path.join(ROOT, "profiles",
                                                                                                   p + "*"))]
    assert not missing, missing


def test_cited_tools_exist():
    missing = [(d, p) for d, p in _refs("tools")
               if p.endswith((".py", ".sh")) and not glob.glob(os.path.join(ROOT, "tools", p))]
    assert not missing, missing


def test_cited_tests_exist():
    """test functions the docs name (a prefix may stand for a parametrised family)"""
    names = set()
    for f in glob.glob(os.path.join(ROOT, "tests", "*.py")):
        names.update(re.findall(r"^def (test_\w+)", open(f).read(), re.M))
    missing = []
    for doc in DOCS:
        for n in re.findall(r"`(test_\w+)", open(os.path.join(ROOT, doc)).read()):
            if not any(x.startswith(n) for x in names):
                missing.append((doc, n))
    assert not missing, missing


def _read_names(paths, pattern):
    return {n for p in paths for n in re.findall(pattern, open(p).read())}


def test_runtime_switch_table_matches_the_environment_reads():
    """INTEGRATION.md §6's table lists exactly the `SK_*` variables the package reads from the environment:
    getenv("SK_...") in csrc/, os.environ / env.get in the Python package and the knob table of
    sk_multi_plan.hpp.  Variables only bench.py reads may be listed too.  A name counts as listed when it stands
    in a row's first cell, not when another row's text mentions it"""
    pkg = os.path.join(ROOT, "skillshot_learning_amd")
    read = _read_names(glob.glob(os.path.join(pkg, "csrc", "*")), r'getenv\(\s*"(SK_\w+)"')
    read |= _read_names([os.path.join(pkg, "csrc", "sk_multi_plan.hpp")], r'\{"(SK_\w+)",\s*&MultiKnobs::')
    env_get = r'(?:\benviron|\benv)(?:\.get\(|\[)\s*"(SK_\w+)"'
    read |= _read_names(glob.glob(os.path.join(pkg, "*.py")), env_get)
    bench_only = _read_names([os.path.join(ROOT, "bench.py")], env_get) - read
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = re.search(r"^## 6\. .*?(?=^## |\Z)", text, re.S | re.M).group(0)
    table = set()
    for row in re.findall(r"^\|([^|]*)\|", section, re.M):
        table.update(re.findall(r"`(SK_\w+)`", row))
    assert read and table
    assert read - table == set(), "read from the environment, no row in the table"
    assert table - read - bench_only == set(), "a row in the table, read nowhere"
