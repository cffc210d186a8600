"""Generate tests/golden/cell_store_refusals.json: what the gh_set_cells_* entry points and the stores behind them
answer the scripted cases of tests/cell_store_cases.py, and the bits of the smallest context of every cell kind.

TEST INFRASTRUCTURE ONLY; the library has no CPU path, so it runs on the GPU machine, on the library whose behaviour is
to be kept (the commit BEFORE a change of the host side that describes the stores):
    python tests/make_golden_cell_refusals.py [output.json] [--values]
GRAVHMC_LIB names another build of the library.  The file holds DATA only: per refusal case the return code and
gh_last_error's text of every step; per bit case SHA-256 digests, kernel_stats() and multi_info().  Two runs on the same
library write the same file (checked when the fixture was made: every quantity reproduced bit for bit); --values adds the
arrays themselves as hex floats, to look at a quantity that does not.
(Not collected by pytest: the name does not start with test_.)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import cell_store_cases as cases  # noqa: E402


def main(argv):
    import gravinv3dhmc_amd as pkg
    from gravinv3dhmc_amd import _lib, engine  # noqa: F401
    args = [a for a in argv if not a.startswith("--")]
    out = args[0] if args else os.path.join(ROOT, "tests", "golden", "cell_store_refusals.json")
    doc = {"refusals": cases.run_refusals(_lib), "bits": cases.run_bits(pkg, values="--values" in argv)}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    n_ref = sum(1 for steps in doc["refusals"].values() for rc, _ in steps if rc != 0)
    print("wrote %s: %d refusal cases (%d refusing steps), %d bit cases"
          % (out, len(doc["refusals"]), n_ref, len(doc["bits"])))


if __name__ == "__main__":
    main(sys.argv[1:])
