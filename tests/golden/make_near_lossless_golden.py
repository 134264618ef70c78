#!/usr/bin/env python3
"""Generates tests/golden/near_lossless.json with the REAL reference (oracle/_ref/libojph_ref.so).  Run where the reference
has been built only:

    python tests/golden/make_near_lossless_golden.py

Per coded case of tests/trunc_cases.py and per DISTINCT level of its truncation ladder (a level whose table differs from the
level before): the squared error and the peak absolute error, per component, between the case's image and what the reference
decodes from the CPU statement's codestream of that level (tests/trunc_cases.cpu_codestream).  Level 0 is checked here to
decode to the image.
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

OUT = os.path.join(HERE, "near_lossless.json")


def main():
    ref = refbind.Ref()
    out = {"cases": {}}
    for name in tc.CODED:
        plan, img, _ = tc.case_state(name)
        levels = tc.distinct_levels(plan)
        sse, pae = [], []
        for j in levels:
            planes, _ = ref.decode(tc.cpu_codestream(name, j))
            d = np.asarray(planes).astype(np.int64) - img.astype(np.int64)
            sse.append([int((d[c] * d[c]).sum()) for c in range(len(d))])
            pae.append([int(np.abs(d[c]).max()) for c in range(len(d))])
        assert not any(sse[0]) and not any(pae[0]), "level 0 of case %s does not decode to the image" % name
        out["cases"][name] = dict(levels=levels, sse=sse, pae=pae)
        print(name, len(levels), [max(p) for p in pae[1:8]], [sum(s) for s in sse[1:4]])
    with open(OUT, "w") as f:
        json.dump(out, f, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
