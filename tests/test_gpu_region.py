"""Region decoding on the GPU: a decoder made for a rectangle writes exactly the crop of the whole-frame decode, for both
wavelets, every container, colour fused or not, reduced resolutions, batches and repeated runs, and it decodes and uploads
only a small part of the codestream for a small region."""
import numpy as np
import pytest

from openjph_amd import codec
from tests.region_cases import CASES, SKIPS, crop, encode_case, random_cs, regions_for

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _frame(dec, dtype):
    return dec.run_device(dtype=dtype).cpu().numpy()


def check_region(cs, region, skip=None, dtypes=(torch.int32,)):
    full = codec.Decoder(cs, skip_res=skip)
    reg = codec.Decoder(cs, skip_res=skip, region=region)
    for dt in dtypes:
        want = crop(full.plan, _frame(full, dt).astype(np.int64), reg.plan)
        assert full.failed_blocks() == 0
        got = reg.plan.unpack_frame(_frame(reg, dt).astype(np.int64))
        assert reg.failed_blocks() == 0
        for c, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a, b), "component %d of region %s (%s) differs" % (c, region, dt)
    return reg


@pytest.mark.parametrize("name,kw,size", CASES, ids=[c[0] for c in CASES])
def test_region_equals_crop_of_full_decode(name, kw, size):
    cs = encode_case(kw, size)
    for r in regions_for(size):
        check_region(cs, r, dtypes=(torch.int32, torch.int16, torch.uint8))


@pytest.mark.parametrize("skip", [s[1] for s in SKIPS], ids=[s[0] for s in SKIPS])
@pytest.mark.parametrize("name", ["rev-L5", "irv-L4", "420", "colour", "colour-irv"])
def test_region_with_skipped_resolutions(name, skip):
    _, kw, size = next(c for c in CASES if c[0] == name)
    cs = encode_case(kw, size)
    for r in regions_for(size, seed=3):
        check_region(cs, r, skip=skip)


@pytest.mark.parametrize("seed", range(8))
def test_region_random_parameter_sets(seed):
    cs, size = random_cs(seed)
    for r in regions_for(size, seed=seed)[:6]:
        check_region(cs, r)


@pytest.mark.parametrize("name", ["colour", "colour-irv"])
def test_region_unfused_colour(name, monkeypatch):
    monkeypatch.setenv("OJPHGPU_NO_COLOUR_FUSION", "1")
    _, kw, size = next(c for c in CASES if c[0] == name)
    cs = encode_case(kw, size)
    for r in regions_for(size, seed=5):
        check_region(cs, r, dtypes=(torch.int32, torch.uint8))


def test_region_nlt3_and_zero_level_component():
    from tests import cpu_pipeline as cp
    from tests.region_cases import planes_for
    size = (83, 71)
    kw = dict(reversible=True, num_decomps=4, is_signed=True, downsampling=[(1, 1), (1, 1)], nlt={"all": 3},
              coc={1: dict(reversible=True, num_decomps=0)})
    planes = [q - 128 for q in planes_for(dict(downsampling=[(1, 1), (1, 1)]), size)]
    cs = cp.encode(planes, size=size, **kw)[0]
    for r in regions_for(size, seed=2):
        check_region(cs, r)


def test_same_decoder_twice_and_batch():
    _, kw, size = next(c for c in CASES if c[0] == "irv-odd-offsets-tiles")
    cs = encode_case(kw, size)
    r = (13, 7, 50, 41)
    dec = check_region(cs, r)
    a = dec.run_device().cpu().numpy(); assert dec.failed_blocks() == 0
    b = dec.run_device().cpu().numpy(); assert dec.failed_blocks() == 0
    assert np.array_equal(a, b)
    batch = codec.Decoder([cs, cs, cs], region=r)
    got = batch.run_device().cpu().numpy()
    assert batch.failed_blocks() == 0
    for f in range(3):
        assert np.array_equal(got[f].reshape(a.shape), a)


def test_small_region_decodes_and_uploads_little():
    cs = encode_case(dict(reversible=True, num_decomps=5, block=(64, 64), tile=(1024, 1024)), (2048, 2048))
    full = codec.Decoder(cs)
    info_full = full.region_info()
    dec = check_region(cs, (900, 900, 64, 64))               # inside the first tile
    info = dec.region_info()
    assert info["plan_blocks"] == info_full["blocks"] == info_full["plan_blocks"]
    assert info["blocks"] < 0.1 * info["plan_blocks"]
    assert info["tiles"] == 1 and info_full["tiles"] == 4
    assert info["upload_bytes"] < 0.1 * len(cs)
    dec2 = check_region(cs, (1000, 1000, 100, 100))          # spans the four tiles
    assert dec2.region_info()["tiles"] == 4


def test_region_decode_host_call():
    _, kw, size = next(c for c in CASES if c[0] == "colour")
    cs = encode_case(kw, size)
    full = codec.decode(cs)
    got = codec.decode(cs, region=(5, 6, 30, 20))
    assert np.array_equal(got, full[:, 6:26, 5:35])
