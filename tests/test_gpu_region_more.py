"""Region decoding on the GPU, continued: the region synthesis kernel as a stage against the oracle's synthesis, full-size
frames, the other block-decoder schedules, resilient decodes of damaged codestreams, the live reference, and the command-line
tool and facade."""
import os
import subprocess
import sys

import numpy as np
import pytest

from openjph_amd import codec
from tests.region_cases import CASES, crop, encode_case, regions_for

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the kernel as a stage -------------------------------------------------------------------------------------------------
def _plane_case(rng, w, h, xe, ye, rev):
    from oracle import oraclebind as ob
    lw, hw, lh, hh = ob.band_dims(w, h, xe, ye)
    dt = np.int32 if rev else np.float32
    bands = [(rng.integers(-300, 300, (rh, rw)) if rev else rng.normal(0, 0.05, (rh, rw))).astype(dt)
             for rw, rh in ((lw, lh), (hw, lh), (lw, hh), (hw, hh))]
    want = (ob.dwt53_inv if rev else ob.dwt97_inv)(*bands, w, h, xe, ye)
    return bands, want


def _desc(bands, w, h, xe, ye, base, arena):
    """bands placed one after another from element `base` of the arena (uint32 numpy), the plane behind them"""
    d = np.zeros(1, codec.dwt_desc_dtype)[0]
    off = base
    for name, b in zip(("ll", "hl", "lh", "hh"), bands):
        d[name + "_off"] = off; d[name + "_pitch"] = max(b.shape[1], 1)
        arena[off:off + b.size] = b.view(np.uint32).ravel()
        off += max(b.size, 1)
    d["src_off"] = off; d["src_pitch"] = w
    d["w"], d["h"], d["x_even"], d["y_even"] = w, h, int(xe), int(ye)
    return d, off + w * h


def _regions(w, h, rng):
    out = [(0, 0, w, h), (0, 0, 1, 1), (w - 1, h - 1, w, h), (w // 2, 0, w, 1), (0, h // 2, 1, h)]
    for _ in range(4):
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        out.append((x0, y0, int(rng.integers(x0 + 1, w + 1)), int(rng.integers(y0 + 1, h + 1))))
    return out


@pytest.mark.parametrize("rev", [True, False], ids=["53", "97"])
@pytest.mark.parametrize("container", [0, 32, 16, 8])
def test_region_kernel_against_oracle_synthesis(rev, container):
    from oracle import oraclebind as ob
    rng = np.random.default_rng(5 + container + rev)
    for w, h in ((1, 17), (17, 1), (2, 2), (131, 77), (300, 45), (61, 260)):
        for xe in (True, False):
            for ye in (True, False):
                bands, want = _plane_case(rng, w, h, xe, ye, rev)
                arena = np.zeros(8 * (w + 2) * (h + 2) + 64, np.uint32)
                d, end = _desc(bands, w, h, xe, ye, 0, arena)
                bd = 8 if container == 8 else 12
                d["reserved"] = bd
                for (x0, y0, x1, y1) in _regions(w, h, rng):
                    rw, rh = x1 - x0, y1 - y0
                    r = np.zeros(1, codec.dwt_region_dtype)
                    r[0]["rx0"], r[0]["ry0"], r[0]["rx1"], r[0]["ry1"] = x0, y0, x1, y1
                    r[0]["out_off"], r[0]["out_pitch"] = 3, rw + 1
                    d_arena = torch.from_numpy(arena.view(np.int32).copy()).cuda()
                    if container == 0:
                        codec.dwt_inverse_region(rev, np.array([d]), r, d_arena)
                        plane = d_arena.cpu().numpy().view(np.uint32)[end - w * h:end].reshape(h, w)
                        got = plane[y0:y1, x0:x1]
                        assert np.array_equal(got, np.ascontiguousarray(want).view(np.uint32)[y0:y1, x0:x1]), (w, h, xe, ye, x0, y0, x1, y1)
                        continue
                    tdt = {32: torch.int32, 16: torch.int16, 8: torch.uint8}[container]
                    img = torch.full((3 + rh * (rw + 1) + 5,), 77, dtype=tdt, device="cuda")
                    codec.dwt_inverse_region(rev, np.array([d]), r, d_arena, img, container)
                    out = img.cpu().numpy().astype(np.int64)
                    if rev:
                        exp = want.astype(np.int64) + (1 << (bd - 1))
                    else:
                        e = np.empty(want.shape, np.int32)
                        ob.lib().ojo_irv_to_int(np.ascontiguousarray(want).ctypes.data, e.ctypes.data, want.size, bd, 0)
                        exp = e.astype(np.int64)
                    if container == 16:
                        exp = np.clip(exp, 0, 65535); out = out & 0xFFFF
                    if container == 8:
                        exp = np.clip(exp, 0, 255)
                    got = out[3:3 + rh * (rw + 1)].reshape(rh, rw + 1)
                    assert np.array_equal(got[:, :rw], exp[y0:y1, x0:x1]), (w, h, xe, ye, x0, y0, x1, y1)
                    assert (got[:, rw] == 77).all() and (out[:3] == 77).all() and (out[3 + rh * (rw + 1):] == 77).all()


def test_region_kernel_colour_triples():
    """NC = 3: three 5/3 planes, the inverse RCT in the stores"""
    rng = np.random.default_rng(9)
    for w, h, xe, ye in ((90, 41, True, False), (33, 70, False, True)):
        cases = [_plane_case(rng, w, h, xe, ye, True) for _ in range(3)]
        arena = np.zeros(3 * 8 * (w + 2) * (h + 2), np.uint32)
        descs, at = [], 0
        for bands, _ in cases:
            d, at = _desc(bands, w, h, xe, ye, at, arena)
            d["reserved"] = 10
            descs.append(d)
        y, cb, cr = [c[1].astype(np.int64) for c in cases]
        g = y - ((cb + cr) >> 2)
        want = [cr + g + 512, g + 512, cb + g + 512]
        for (x0, y0, x1, y1) in _regions(w, h, rng):
            rw, rh = x1 - x0, y1 - y0
            r = np.zeros(3, codec.dwt_region_dtype)
            for k in range(3):
                r[k]["rx0"], r[k]["ry0"], r[k]["rx1"], r[k]["ry1"] = x0, y0, x1, y1
                r[k]["out_off"], r[k]["out_pitch"] = k * rw * rh, rw
            img = torch.zeros(3 * rw * rh, dtype=torch.int32, device="cuda")
            codec.dwt_inverse_region(True, np.array(descs), r, torch.from_numpy(arena.view(np.int32).copy()).cuda(), img, 32, colour=True)
            out = img.cpu().numpy().reshape(3, rh, rw)
            for k in range(3):
                assert np.array_equal(out[k], want[k][y0:y1, x0:x1])


# ---- whole decoder ---------------------------------------------------------------------------------------------------------
def test_region_against_oracle_pipeline_and_reference():
    """independent of the library's own whole-frame decoder: the oracle pipeline's decode, and the live reference where built"""
    from oracle import refbind
    from tests import cpu_pipeline as cp
    from openjph_amd.plan import parse_codestream
    for name in ("irv-L5", "odd-offsets-tiles", "colour", "422-irv"):
        _, kw, size = next(c for c in CASES if c[0] == name)
        cs = encode_case(kw, size)
        want, full = cp.decode(cs)
        ref = None                                      # (9/7: the generic build is the bit-exact one)
        generic = not kw.get("reversible", True)
        if refbind.available(generic=generic):
            ref, _ = refbind.Ref(generic=generic).decode(cs)
        for r in regions_for(size, seed=11)[:6]:
            dec = codec.Decoder(cs, region=r)
            got = dec.plan.unpack_frame(dec.decode())
            for a, b in zip(got, crop(full, want, dec.plan)):
                assert np.array_equal(a, b), (name, r)
            if ref is not None:
                for a, b in zip(got, crop(full, ref, dec.plan)):
                    assert np.array_equal(a, b), (name, r, "reference")


@pytest.mark.parametrize("env", [{"OJPHGPU_DEC_FUSED": "0"}, {"OJPHGPU_DEC_PREP": "1"}, {"OJPHGPU_DEC_FUSED": "2"},
                                 {"OJPHGPU_DEC_FUSED": "2", "OJPHGPU_FUSED_SHAPE": "0"}, {"OJPHGPU_DEC_FUSED": "2", "OJPHGPU_FUSED_RINGS": "1"},
                                 {"OJPHGPU_NO_OVERLAP": "1"}],
                         ids=["separate-launches", "prep-launch", "fused-wherever-possible", "fused-8-wavefront-shape",
                              "fused-one-ring-per-wavefront", "no-overlap"])
def test_region_under_the_other_decoder_schedules(env):
    script = r'''
import sys, numpy as np
sys.path.insert(0, %r)
from openjph_amd import codec
from tests import cpu_pipeline as cp
from tests.region_cases import crop
from tests.synth import synth_image
for kw, shape, r in ((dict(bit_depth=8, num_decomps=3), (1, 333, 517), (101, 37, 200, 150)),
                     (dict(bit_depth=12, reversible=False, qstep=0.002, tile=(256, 192)), (3, 401, 611), (250, 180, 90, 40)),
                     (dict(bit_depth=10, block=(32, 32)), (1, 200, 300), (7, 9, 1, 120))):
    img = synth_image(shape[0], shape[1], shape[2], kw["bit_depth"], seed=11)
    cs = codec.encode(img, **kw)
    want, full = cp.decode(cs)
    dec = codec.Decoder(cs, region=r)
    for _ in range(2):
        got = dec.plan.unpack_frame(dec.run_device().cpu().numpy())
        assert dec.failed_blocks() == 0
        for a, b in zip(got, crop(full, want, dec.plan)):
            assert np.array_equal(a, b), kw
print("OK")
''' % ROOT
    r = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0 and b"OK" in r.stdout, r.stderr[-2000:]


def test_resilient_region_of_damaged_codestreams():
    """resilient decodes of damaged codestreams (padded blocks, failed blocks): the region is the crop of the whole decode"""
    from tests import damaged_cases
    compared = 0
    for name, cs in damaged_cases.cases():
        try:
            full = codec.Decoder(cs, resilient=True)
            whole = full.run_device().cpu().numpy(); full.failed_blocks()
        except Exception:
            continue
        if full.plan.frame_elems == 0:
            continue
        W, H = int(full.plan.params.width), int(full.plan.params.height)
        for r in ((0, 0, W, H), (W // 3, H // 4, max(W // 2, 1), max(H // 2, 1))):
            dec = codec.Decoder(cs, resilient=True, region=r)
            got = dec.plan.unpack_frame(dec.run_device().cpu().numpy())
            dec.failed_blocks()
            for a, b in zip(got, crop(full.plan, whole, dec.plan)):
                assert np.array_equal(a, b), (name, r)
        compared += 1
        if compared >= 24:
            break
    assert compared >= 8


# ---- full size ------------------------------------------------------------------------------------------------------------
def test_c3_8k_region():
    from tests.test_gpu_fullsize import GOLD, coded, sha
    img, cs, dec = coded("c3")
    assert sha(dec.astype(np.int32)) == GOLD["c3"]["generic"]["decoded_sha256"]
    r = codec.Decoder(cs, region=(1001, 1333, 1024, 1024))
    got = r.decode()
    assert np.array_equal(got, dec[:, 1333:1333 + 1024, 1001:1001 + 1024])
    info = r.region_info()
    assert info["upload_bytes"] < 0.1 * len(cs) and info["blocks"] < info["plan_blocks"] // 4


def test_c4_16k_region_across_tiles():
    from tests import synth
    from tests.test_gpu_fullsize import GOLD, sha
    from openjph_amd.plan import Plan, make_params
    g = GOLD["c4"]
    img = synth.survey_c4()
    plan = Plan(make_params(16384, 16384, 1, bit_depth=16, tile=(1024, 1024)))
    cs = codec.Encoder(plan=plan).encode(img)
    assert sha(cs) == g["sha256"]
    x0, y0, w, h = 3000, 5000, 2500, 1700
    r = codec.Decoder(cs, region=(x0, y0, w, h))
    got = r.decode()
    assert np.array_equal(got[0], img[0, y0:y0 + h, x0:x0 + w])       # the whole decode is lossless: img is its output
    info = r.region_info()
    assert info["tiles"] <= 12 and info["upload_bytes"] < 0.1 * len(cs)


# ---- command line and facade -----------------------------------------------------------------------------------------------
EXPAND = os.path.join(ROOT, "openjph_amd", "apps", "ojph_expand")


def _run(cmd):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)


def test_cli_region(tmp_path):
    from tests import cpu_pipeline as cp
    from tests.synth import synth_image
    from tests.test_cli import read_pnm
    for nc, ext in ((1, ".pgm"), (3, ".ppm"), (3, ".raw")):
        img = synth_image(nc, 150, 230, 8, seed=5)
        cs, *_ = cp.encode(img, bit_depth=8, color_transform=nc == 3, num_decomps=4)
        j2c = tmp_path / "a.j2c"
        open(j2c, "wb").write(cs)
        for skip, reg in ((None, (13, 21, 100, 61)), ((1, 1), (13, 21, 100, 61)), ((2, 1), (0, 0, 230, 150))):
            out = tmp_path / ("o" + ext)
            cmd = [EXPAND, "-i", str(j2c), "-o", str(out), "-region", "%d,%d,%d,%d" % reg]
            if skip:
                cmd += ["-skip_res", "{%d,%d}" % skip]
            res = _run(cmd)
            assert res.returncode == 0, res.stdout
            want, _ = cp.decode(cs, skip=skip)
            f = 1 << (skip[1] if skip else 0)
            x0, y0 = -(-reg[0] // f), -(-reg[1] // f)
            x1, y1 = -(-(reg[0] + reg[2]) // f), -(-(reg[1] + reg[3]) // f)
            want = np.clip(np.asarray(want)[:, y0:y1, x0:x1], 0, 255)
            if ext == ".raw":
                # (the raw writer keeps the low byte of a sample out of range: against the crop of the tool's own
                # whole-frame .raw, whose samples the other CLI tests pin)
                full_cmd = [EXPAND, "-i", str(j2c), "-o", str(tmp_path / "full.raw")] + (["-skip_res", "{%d,%d}" % skip] if skip else [])
                assert _run(full_cmd).returncode == 0
                fh, fw = -(-150 // f), -(-230 // f)
                full = np.frombuffer(open(tmp_path / "full.raw", "rb").read(), np.uint8).reshape(nc, fh, fw)
                want = full[:, y0:y1, x0:x1]
                got = np.frombuffer(open(out, "rb").read(), np.uint8).reshape(want.shape)
            else:
                got = read_pnm(out)
            assert np.array_equal(got, want), (ext, skip, reg)
    res = _run([EXPAND, "-i", str(j2c), "-o", str(tmp_path / "o.ppm"), "-region", "0,0,231,1"])
    assert res.returncode != 0 and b"ojph error" in res.stdout


def test_facade_pulls_region_lines(tmp_path):
    from tests import cpu_pipeline as cp
    from tests.region_cases import planes_for
    exe = os.path.join(ROOT, "openjph_amd", "apps", "facade_region_lines")
    size = (91, 67)
    planes = planes_for(dict(downsampling=[(1, 1), (2, 2), (2, 2)], image_offset=(1, 1)), size)
    cs = cp.encode(planes, size=size, num_decomps=3, downsampling=[(1, 1), (2, 2), (2, 2)], image_offset=(1, 1))[0]
    j2c = tmp_path / "r.j2c"
    open(j2c, "wb").write(cs)
    for args in (["5", "7", "40", "33"], ["0", "0", "91", "67"], ["60", "3", "31", "64", "1"]):
        res = _run([exe, str(j2c)] + args)
        assert res.returncode == 0, res.stdout
