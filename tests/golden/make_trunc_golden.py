#!/usr/bin/env python3
"""Generates tests/golden/trunc.json with the REAL reference (oracle/_ref/libojph_ref.so).  Run where the reference has been
built only:

    python tests/golden/make_trunc_golden.py

Per coded case of tests/trunc_cases.py and per level of its truncation ladder: the length and SHA-256 of the CPU statement's
codestream (tests/trunc_cases.cpu_truncated) and the SHA-256 of the planes the reference decodes from it (int32, component
after component).  Level 0 is checked here to be the reference's own encode, byte for byte.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import refbind                      # noqa: E402
from tests import trunc_cases as tc             # noqa: E402

OUT = os.path.join(HERE, "trunc.json")


def main():
    ref = refbind.Ref()
    out = {"cases": {}}
    for name in tc.CODED:
        plan, img, _ = tc.case_state(name)
        J = plan.trunc_levels
        want = ref.encode(img, **tc.CASES[name]["kw"])
        assert want == tc.cpu_codestream(name, 0), "level 0 of case %s is not the reference's encode" % name
        sizes, cs_sha, dec_sha = [], [], []
        for j in range(J):
            cs = tc.cpu_codestream(name, j)
            planes, _ = ref.decode(cs)
            sizes.append(len(cs)); cs_sha.append(tc.sha(cs))
            dec_sha.append(tc.sha(np.ascontiguousarray(planes, dtype=np.int32).tobytes()))
        out["cases"][name] = dict(levels=J, sizes=sizes, codestream_sha256=cs_sha, decoded_sha256=dec_sha)
        print(name, J, sizes[0], sizes[-1])
    with open(OUT, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
