"""Generate tests/golden/module_layer.json: what the inversion modules and HMCSampleBatch answer the scripted cases of
tests/module_layer_cases.py.

TEST INFRASTRUCTURE ONLY; run on the commit whose behaviour is to be kept (the one BEFORE a change of the module layer,
with the case file copied onto it):
    python tests/make_golden_module_layer.py [output.json]
The host part needs neither a GPU nor the library; the device part does, so it runs on the GPU machine (GRAVHMC_LIB
names another build of the library).  The file holds DATA only: exception class names and texts, printed lines,
warnings, attribute names with type and shape, and SHA-256 digests (their first 16 hex digits).  Two runs on the same
package write the same file (checked when the fixture was made: every quantity reproduced bit for bit).
(Not collected by pytest: the name does not start with test_.)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import module_layer_cases as cases  # noqa: E402


def main(argv):
    args = [a for a in argv if not a.startswith("--")]
    out = args[0] if args else os.path.join(ROOT, "tests", "golden", "module_layer.json")
    doc = {"host": cases.run_host(), "device": cases.run_device()}
    forms = {}      # what vars(module) holds, written once for the cases that share it
    for k, v in sorted(doc["device"].items()):
        if "vars" in v:
            forms.setdefault(v.pop("vars"), []).append(k)
    with open(out, "w") as f:      # one line per host case and per quantity of a device case
        host = ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in sorted(doc["host"].items()))
        device = ",\n".join(" %s: {\n%s\n }" % (json.dumps(k), ",\n".join(
            "  %s: %s" % (json.dumps(q), json.dumps(x)) for q, x in sorted(v.items())))
            for k, v in sorted(doc["device"].items()))
        held = ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in sorted(forms.items()))
        f.write('{"host": {\n%s\n},\n"device": {\n%s\n},\n"vars": {\n%s\n}}\n' % (host, device, held))
    quiet = [k for k, v in doc["host"].items() if not v]
    print("wrote %s: %d host cases (%d raise nothing), %d device cases" % (out, len(doc["host"]), len(quiet),
                                                                          len(doc["device"])))


if __name__ == "__main__":
    main(sys.argv[1:])
