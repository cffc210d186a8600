"""Host suite of the inversion modules' constructors and of HMCSampleBatch's refusals: everything they decide before an
Engine exists, so it runs without a GPU and without the library.

The yardstick is the "host" part of tests/golden/module_layer.json, recorded by tests/make_golden_module_layer.py from
the scripted cases of tests/module_layer_cases.py on the package as it was before the modules' shared parts were written
once (inversion/potential.py).  Compared EXACTLY: the exception's class name and its text -- with
two faults in one call, the text tells the order of the checks."""
import json
import os

import pytest

import module_layer_cases as cases
from conftest import GOLD


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLD, "module_layer.json")) as f:
        return json.load(f)["host"]


def test_the_host_cases_are_the_recorded_ones(golden):
    assert sorted(name for name, _ in cases.host_cases()) == sorted(golden)
    assert all(v.split(": ")[0] in ("ValueError", "TypeError", "NotImplementedError") and v.split(": ", 1)[1]
               for v in golden.values())


def test_refusals_classes_and_texts(golden):
    got = cases.run_host()
    bad = ["%s:\n    recorded %r\n    got      %r" % (name, want, got.get(name))
           for name, want in sorted(golden.items()) if got.get(name) != want]
    print("module layer, host: %d cases, %d differ" % (len(got), len(bad)))
    assert not bad, "\n".join(bad)
