"""A quality target under a byte cap through the command-line tool (ojph_compress -min_psnr dB -cap_bytes N, which goes
through ojph::codestream::set_max_sse(max_sse, cap_bytes) and get_capped_info of the facade): frame A of tests/rate_cases.py
as a .ppm, both outcomes, against the Python encoder, and the two error messages."""
import os
import re
import subprocess

import numpy as np
import pytest

from openjph_amd.plan import make_params
from tests import capped_cases as cc
from tests import rate_cases as rc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPRESS = os.path.join(ROOT, "openjph_amd", "apps", "ojph_compress")


def run(cmd):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)


def test_cli_min_psnr_under_cap_bytes(tmp_path):
    from openjph_amd import codec
    name = "A"
    c = rc.CASES[name]
    img, _ = rc.case_image(name)
    src = tmp_path / "a.ppm"
    with open(src, "wb") as f:
        f.write(b"P6\n%d %d\n%d\n" % (c["w"], c["h"], (1 << c["bd"]) - 1))
        f.write(np.ascontiguousarray(img.transpose(1, 2, 0)).astype(">u2").tobytes())
    params = make_params(c["w"], c["h"], c["nc"], **rc.case_kwargs(name))
    T = cc.QUAL["cases"][name]["targets"]["50"]["max_sse"]
    total, sizes = cc.tables(name)
    inr, below, _ = rc.budgets(name)
    common = ["-i", str(src), "-reversible", "false", "-num_decomps", "4"]
    seen = set()
    for cap in (inr[1], inr[2]):
        out = tmp_path / ("out%d.j2c" % cap)
        r = run([COMPRESS, "-o", str(out), "-min_psnr", "50", "-cap_bytes", str(cap)] + common)
        text = r.stdout.decode()
        assert r.returncode == 0, text
        enc = codec.Encoder(params, max_sse=T, cap_bytes=cap)
        want = enc.encode(img)
        info = enc.capped_info()
        assert open(out, "rb").read() == want and len(want) <= cap
        assert (info["grid_index"], info["outcome"]) in cc.answers(total, sizes, T, cap)
        m = re.search(r"max_sse (\d+), outcome (\w+), .*grid index (\d+), the target's (\d+)\), sse (\d+), .* (\d+) quality trials, (\d+) codings", text)
        assert m, text
        assert int(m.group(1)) == T and m.group(2) == ("MET", "BY_BUDGET")[info["outcome"]]
        assert [int(m.group(k)) for k in (3, 4, 5)] == [info["grid_index"], info["quality_index"], info["sse"]]
        assert (int(m.group(6)), int(m.group(7))) == (info["quality_passes"], info["rate_passes"])
        seen.add(m.group(2))
    assert seen == {"MET", "BY_BUDGET"}
    bad = tmp_path / "bad.j2c"
    r = run([COMPRESS, "-o", str(bad), "-cap_bytes", str(inr[1])] + common)
    assert r.returncode != 0 and b"-cap_bytes" in r.stdout and b"needs -min_psnr" in r.stdout, r.stdout
    r = run([COMPRESS, "-o", str(bad), "-min_psnr", "50", "-max_bytes", str(inr[1])] + common)
    assert r.returncode != 0 and b"-min_psnr and -max_bytes cannot be used together" in r.stdout, r.stdout
    r = run([COMPRESS, "-o", str(bad), "-min_psnr", "50", "-cap_bytes", str(below)] + common)    # nothing fits: the tool fails
    assert r.returncode != 0 and b"byte budget" in r.stdout, r.stdout
    assert not os.path.exists(bad) or os.path.getsize(bad) == 0
