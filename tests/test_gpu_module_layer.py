"""GPU suite of what a constructed inversion module prints, warns, carries and answers, for every branch of the six
constructors (GravMagModule, JointModule, MultiComponentModule, TesseroidMultiComponentModule, MagVectorModule,
TesseroidMagVectorModule).

The yardstick is the "device" part of tests/golden/module_layer.json, recorded by tests/make_golden_module_layer.py from
the scripted cases of tests/module_layer_cases.py on the package as it was before the modules' shared parts were written
once.  Everything is compared EXACTLY: the lines printed with verbose=True (the seconds masked), the warnings, the names
of vars(module) with type and shape, the SHA-256 (its first 16 hex digits) of the weighting's diagonals, of weights,
dobs, dobsw, Aw, A and every kernel(...) form, of forward() and of all five outputs of misfit_and_grad for each
regulariser, block_means(), and the texts of what refuses -- A and kernel on the table forms, Smoothness and TV on a
carved mesh, HMCSampleBatch.  Two runs of the generator on the recording package agreed in every digest, so no quantity
needs a tolerance."""
import json
import os

import pytest

import module_layer_cases as cases
from conftest import GOLD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLD, "module_layer.json")) as f:
        doc = json.load(f)
    for held, names in doc["vars"].items():     # (written once for the cases that share it)
        for name in names:
            doc["device"][name]["vars"] = held
    return doc["device"]


CASES = cases.device_cases()


def test_the_device_cases_are_the_recorded_ones(golden):
    assert sorted(c[0] for c in CASES) == sorted(golden)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_module_as_recorded(built_lib, golden, case):
    got = cases.run_device_case(case)
    want = golden[case[0]]
    bad = ["%s:\n    recorded %r\n    got      %r" % (k, want.get(k), got.get(k))
           for k in sorted(set(want) | set(got)) if want.get(k) != got.get(k)]
    print("module layer [%s]: %d quantities, %d differ" % (case[0], len(got), len(bad)))
    assert not bad, "\n".join(bad)
