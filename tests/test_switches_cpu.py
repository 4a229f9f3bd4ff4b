"""The environment switches of libhybkf.so live in one table (csrc/kf_switches.h): nothing else consults the environment, DESIGN.md lists the
same names, and every name the form suites set is one of them."""
import ast
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "hybkinectfu_amd", "csrc")


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def table_names():
    names = re.findall(r'^\s*(?:X|KF_SWITCH_EXP)\((?:X,\s*)?\w+,\s*"(KF_[A-Z0-9_]+)"', _read(os.path.join(CSRC, "kf_switches.h")), re.M)
    assert names and len(names) == len(set(names)), names
    return set(names)


def tuple_in(module, name):
    """The tuple of strings `name` is assigned at the top level of tests/<module> (read, not imported: the GPU suites load the library)."""
    for node in ast.parse(_read(os.path.join(HERE, module))).body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == name for t in node.targets):
            return ast.literal_eval(node.value)
    raise AssertionError(f"{name} not found in {module}")


def test_only_the_table_reads_the_environment():
    users = []
    for f in sorted(os.listdir(CSRC)):                      # every file, objects of an earlier build included: read as bytes
        path = os.path.join(CSRC, f)
        if os.path.isfile(path):
            with open(path, "rb") as fh:
                if b"getenv(" in fh.read():
                    users.append(f)
    assert users == ["kf_switches.h"], users


def test_design_lists_the_tables_switches():
    design = _read(os.path.join(ROOT, "DESIGN.md"))
    m = re.search(r"^## [^\n]*Switches[^\n]*\n(.*?)(?=^## |\Z)", design, re.M | re.S)
    assert m, "DESIGN.md has no Switches section"
    listed = set(re.findall(r"`(KF_[A-Z0-9_]+)`", m.group(1)))
    assert listed == table_names(), sorted(listed ^ table_names())


def test_every_switch_the_suites_set_is_in_the_table():
    table = table_names()
    for module, name in (("test_gpu_fusion_forms.py", "SWITCHES"), ("test_gpu_raycast_forms.py", "RC_SWITCHES"), ("conftest.py", "FORM_KNOBS")):
        names = tuple_in(module, name)
        assert names and all(isinstance(n, str) for n in names), (module, name)
        missing = [n for n in names if n not in table]
        assert not missing, (module, name, missing)
