"""The two build recipes name the same translation units, and every source file of csrc/ is known to them: mppi-tf_amd/build.py (UNITS,
HEADERS: what source_sha() and stale() look at) and CMakeLists.txt (mppi_unit lines) are kept in step by hand. No compiler, no GPU."""
import glob
import importlib.util
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "mppi-tf_amd", "csrc")


def build_module():
    spec = importlib.util.spec_from_file_location("mppi_build_recipe", os.path.join(ROOT, "mppi-tf_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cmake_units():
    """(source, stem) of every mppi_unit(...) call of CMakeLists.txt, the calls inside a foreach(var values...) once per value"""
    out, loop = [], None
    for line in open(os.path.join(ROOT, "CMakeLists.txt")):
        line = line.split("#")[0].strip()
        m = re.match(r"foreach\((\w+)\s+(.*)\)$", line)
        if m:
            loop = (m.group(1), m.group(2).split())
        elif line.startswith("endforeach"):
            loop = None
        m = re.match(r"mppi_unit\((\S+)\s+(\S+?)[\s)]", line)
        if m:
            var, values = loop if loop else ("", [""])
            out += [tuple(g.replace("${%s}" % var, v) for g in m.groups()) for v in values]
    return out


def test_cmake_builds_the_units_of_build_py():
    units = [(src, stem) for src, _, stem in build_module().UNITS]
    cmake = cmake_units()
    assert len(set(units)) == len(units) and len(set(cmake)) == len(cmake), "a unit is listed twice"
    assert len({stem for _, stem in units}) == len(units), "two units share an object stem"
    assert sorted(cmake) == sorted(units)


def test_every_header_is_a_dependency():
    headers = sorted(os.path.basename(p) for pat in ("*.h", "*.inc") for p in glob.glob(os.path.join(CSRC, pat)))
    assert headers and sorted(build_module().HEADERS) == headers


def test_every_source_is_a_unit():
    sources = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.hip")))
    assert sources and sorted({src for src, _, _ in build_module().UNITS}) == sources
