#!/usr/bin/env python3
"""Generates tests/golden/transcode.json from the REAL reference's generic build (oracle/_ref/libojph_refgen.so) and the
oracle pipeline.  Run where the reference has been built only:

    python tests/golden/make_transcode_golden.py

Per case of tests/transcode_cases.py: the SHA-256 and length of the reference's source codestream; per target the SHA-256
and length of the expected output -- for the identity targets the REFERENCE's direct encode of the original image with the
output parameters, for the others cpu_transcode's output; per irreversible case the length of cpu_transcode's output at
every step of the rate grid, and per budget of rate_cases.budgets the largest index that fits with size(j*), size(j* + 1).
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import refbind                      # noqa: E402
from tests import rate_cases as rc              # noqa: E402
from tests import transcode_cases as tc         # noqa: E402

OUT = os.path.join(HERE, "transcode.json")


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def main():
    refgen = refbind.Ref(generic=True)
    out = {"reference": "aous72/OpenJPH 0.31.0, generic build (oracle/_ref/libojph_refgen.so)", "cases": {}}
    for name, rev in tc.CASES:
        img, size = rc.case_image(name)

        def ref_encode(kw):
            return refgen.encode(img, size=size if isinstance(img, list) else None, **kw)
        cs = ref_encode(tc.src_kwargs(name, rev))
        assert cs == tc.cpu_encode(name, tc.src_kwargs(name, rev)), "the oracle pipeline does not write the reference's source"
        _, arena = tc.cpu_source_planes(cs)
        entry = {"source": {"sha256": sha(cs), "len": len(cs)}, "targets": {}}
        for tg, (_, _, identity) in tc.targets(rev).items():
            kw = tc.out_kwargs(name, rev, tg)
            got = tc.cpu_transcode_planes(arena, tc.case_params(name, kw))
            want = ref_encode(kw) if identity else got
            assert got == want, (name, rev, tg, "cpu_transcode is not the reference's direct encode")
            entry["targets"][tg] = {"sha256": sha(want), "len": len(want), "identity": bool(identity)}
        if not rev:
            sizes = [len(tc.cpu_transcode_planes(arena, tc.case_params(name, tc.out_kwargs(name, rev, "frac", rc.grid_qstep(j)))))
                     for j in range(rc.GRID)]
            inr, below, above = rc.budgets(name)
            assert below < sizes[0] and above > max(sizes)
            entry["sizes"] = sizes
            entry["budgets"] = {}
            for b in inr:
                j = max(k for k in range(rc.GRID) if sizes[k] <= b)
                assert j + 1 < rc.GRID and sizes[j + 1] > b
                entry["budgets"][str(b)] = {"j": j, "bytes": sizes[j], "bytes_finer": sizes[j + 1]}
        out["cases"][tc.case_id(name, rev)] = entry
        print(tc.case_id(name, rev), entry["source"]["len"], {k: v["len"] for k, v in entry["targets"].items()},
              {b: v["j"] for b, v in entry.get("budgets", {}).items()}, flush=True)
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
