#!/usr/bin/env python3
"""Generate tests/golden/create_errors.json: what yl_create answers to every case of tests/_create_cases.py.

    python tests/golden/make_create_fixtures.py          (on a machine with a HIP device)

Run ONCE, at the commit before yl_create's validation moved into the host unit (csrc/yl_program.cpp), with that commit's
library: the file pins the statuses and message texts the refactored validation must keep.  That library reaches its
checks only behind a usable device, hence the GPU machine; YOLOLITE_HIP_LIB selects a library other than the in-tree one.
Stored per case: [status, message]; under "valid": the status of every unedited base program.  Asserted here, so that a
file that pins nothing is never written: every case fails with a message, and the distinct message texts (the "layer N: "
prefix removed) number at least _create_cases.MESSAGE_TEXTS."""
import json
import os
import re
import sys

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from _create_cases import BASES, CASES, MESSAGE_TEXTS, build_case, create  # noqa: E402
from yololite_amd import _lib  # noqa: E402

OUT = os.environ.get("YL_FIXTURE_OUT") or HERE


def main():
    lib = _lib.load()
    rec = {"valid": {}, "cases": {}}
    for base in BASES:
        d, keep = build_case(base)
        st, msg, h = create(lib, d)
        if h:
            lib.yl_destroy(h)
        assert st == _lib.YL_OK, (base, st, msg)
        rec["valid"][base] = st
    for name, base, edit in CASES:
        d, keep = build_case(base, edit)
        st, msg, h = create(lib, d)
        if h:
            lib.yl_destroy(h)
        assert st != _lib.YL_OK and msg, (name, st, msg)
        rec["cases"][name] = [st, msg]
        print(name, st, msg)
    texts = {re.sub(r"^layer \d+: ", "", m) for _, m in rec["cases"].values()}
    assert len(texts) >= MESSAGE_TEXTS, (len(texts), MESSAGE_TEXTS)
    with open(os.path.join(OUT, "create_errors.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("cases", len(rec["cases"]), "distinct texts", len(texts))


if __name__ == "__main__":
    main()
