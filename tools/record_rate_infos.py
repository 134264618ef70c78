"""Records what the budgeted encoders report -- rate_info() in all six fields and rate_rounds(), of the single encoder over
cases A to E and of the batches A, C, E, B (tests/test_gpu_rate_infos.py: measure) -- into
tests/golden/rate_search_infos.json.  Run it on a GPU, from the commit whose search is the one to keep; the test then holds
every later commit to it.
  python tools/record_rate_infos.py [--out tests/golden/rate_search_infos.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "rate_search_infos.json"))
    a = ap.parse_args()
    from tests.test_gpu_rate_infos import measure
    got = measure()
    with open(a.out, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d single and %d batch entries -> %s" % (sum(len(v) for v in got["single"].values()), len(got["batch"]), a.out))


if __name__ == "__main__":
    main()
