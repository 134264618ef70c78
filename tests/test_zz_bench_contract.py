"""The live halves of the bench contract (tests/test_bench_contract.py holds check_line and the CPU half).  This file sorts
LAST on purpose: under `pytest -m gpu -x` every parity test runs before a formatting assertion of the bench line can stop
the run (round 5: one stale label here hid 761 parity tests from the driver)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_bench_contract import ROOT, check_line


@pytest.mark.gpu
def test_live_bench_line():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline", "--e2e-frames", "8"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1                                          # ONE JSON line on stdout
    d = json.loads(lines[0])
    check_line(d, want_cpu_baseline=False)
    assert d["steps"] == 3 and d["warmup"] == 1 and d["config"]["roundtrip_max_abs_err"] <= 8
    assert d["e2e"]["frames"] == 8 and d["e2e_steady_Msamples_s"]["encode"] > 0 and d["e2e_steady_Msamples_s"]["encode+decode"] > 0


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    """without --full a run times exactly --steps steps and prints the headline fields and nothing that takes runs of its own;
    --dump-outputs writes what the last timed step computed: on the C1 frame the reference's codestream (KA-1,
    tests/golden/golden.json) and the frame itself (5/3 reversible: lossless)"""
    from tests.synth import c1_image
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "c1_256_gray_8b_rev53", "--steps", "7", "--warmup", "2",
                        "--dump-outputs", str(tmp_path / "out")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 7 and d["warmup"] == 2 and d["n_gpus"] == 1 and d["config"]["workload"] == "c1_256_gray_8b_rev53"
    assert d["unit"] == "Msamples/s" and d["higher_is_better"] is True and d["dtype"] == "i32" and isinstance(d["metric"], str)
    assert d["ms_per_step"] > 0 and abs(d["value"] - 256 * 256 / d["ms_per_step"] / 1e3) / d["value"] < 1e-3
    assert not {"roofline", "kernels", "verified_after_timing", "e2e", "strong_scaling_c4", "cpu_baseline"} & set(d)
    assert sorted(os.listdir(tmp_path / "out")) == ["codestream.npy", "decoded.npy"]
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "golden.json")))["ka1"]
    cs = np.load(tmp_path / "out" / "codestream.npy")
    assert cs.dtype == np.float32 and len(cs) == gold["len"]
    assert hashlib.sha256(cs.astype(np.uint8).tobytes()).hexdigest() == gold["sha256"]
    dec = np.load(tmp_path / "out" / "decoded.npy")
    assert dec.dtype == np.float32 and np.array_equal(dec, c1_image().reshape(-1).astype(np.float32))


@pytest.mark.gpu
def test_two_ranks_self_launched_on_one_gpu():
    """the N > 1 path of bench.py end to end on the one GPU of the test box: `--gpus 2` starts two ranks itself (both on
    cuda:0, control and gather traffic over gloo), the line says n_gpus 2, and the tile-sharded 16K frame the two ranks
    assemble is byte-identical to the reference's codestream (digest in tests/golden/survey_ka.json)"""
    env = dict(os.environ, OJPH_BENCH_BACKEND="gloo", OJPH_BENCH_ONE_GPU="1")
    env.pop("WORLD_SIZE", None); env.pop("RANK", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--full", "--no-cpu-baseline"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1200, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    check_line(d, want_cpu_baseline=False)
    assert d["n_gpus"] == 2 and len(d["per_rank_ms_per_step"]) == 2 and d["dist"]["world_size"] == 2
    assert d["config"]["frames_per_step"] == 2 and d["scaling"] == "weak"
    s = d["strong_scaling_c4"]
    assert s["n_gpus"] == 2 and s["tiles_per_rank"] == [128, 128] and len(s["per_rank_ms_per_step"]) == 2
    assert s["codestream_equals_reference_digest"] is True and s["tiles_lossless_on_every_rank"] is True
    assert s["gather"]["bytes_received_by_rank0"] > 100e6 and s["value"] > 0
    # the two end-to-end forms of the gather: tile-parts sent to rank 0 (gatherv), and every rank placing its own in ONE shared
    # host segment (shard.HostGather, the default of shard.encode_sharded on one node) -- both must be the reference's bytes
    e = s["e2e_encode"]
    assert e["codestream_equals_reference_digest"] is True and e["ms"] > 0
    hs = e["shared_host_segment"]
    assert "error" not in hs, hs
    assert hs["codestream_equals_reference_digest"] is True and hs["ms"] > 0 and hs["Msamples_s"] > 0
