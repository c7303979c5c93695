"""Which template instance a K1 launch runs, over the whole input space of each tuned family's decision (CPU-side, no GPU).

csrc/k1_instance.h is the one place that decides: enqueue_grad_once arms what the decided instance needs and the launchers look the
decided flags up in tables built from the header's instance lists.  tests/golden/k1_instances.json was recorded from the launchers'
ladders of `if`s before the decision moved there (inputs no context reaches included: the functions are total).  This compiles
k1_instances_table.cpp -- the header alone, with a host compiler -- and compares what it prints, line by line."""
import json
import os
import shutil
import subprocess

import pytest

import __graft_entry__ as g

HERE = os.path.dirname(os.path.abspath(__file__))
INSTANCES = {"f16_v8": 24, "f16_k128": 8, "f16_k32": 4, "bf16_v7": 5, "f32_pc": 8}      # kernels instantiated per family


def _host_compiler():
    for cand in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++")):
        if cand and os.path.exists(cand):
            return [cand]
    try:
        return [g._hipcc(), "-x", "c++"]
    except RuntimeError:
        pytest.skip("no host C++ compiler")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("k1_instances") / "table")
    cmd = _host_compiler() + ["-std=c++17", "-O1", "-I", g.CSRC, os.path.join(HERE, "k1_instances_table.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    rows = {}
    for line in out.splitlines():
        family, key, flags, has = line.split("\t")
        rows.setdefault(family, {})[key] = (flags, has)
    return rows


def test_decision_matches_the_recorded_ladders(table):
    with open(os.path.join(HERE, "golden", "k1_instances.json")) as f:
        golden = json.load(f)["instances"]
    assert sorted(golden) == sorted(INSTANCES)
    for family, want in golden.items():
        got = {key: flags for key, (flags, _) in table[family].items()}
        assert sorted(got) == sorted(want), family
        wrong = {key: (got[key], want[key]) for key in want if got[key] != want[key]}
        assert not wrong, "%s: %d inputs decide another instance (got, recorded), e.g. %s" % (family, len(wrong), sorted(wrong.items())[:4])


def test_every_decided_flag_set_is_an_instance(table):
    for family, n in INSTANCES.items():
        missing = sorted(key for key, (_, has) in table[family].items() if has != "1")
        assert not missing, "%s: no line in the launcher's instance table for %s" % (family, missing[:4])
        assert len({flags for flags, _ in table[family].values()}) == n, family      # and every instance is decided by some input


def test_switches_are_on_unless_zero(table):
    assert table["switches"] == {"011": ("011", "1")}
