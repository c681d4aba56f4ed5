"""CPU: the PNG decoder (stp3_amd.datas.PngDecoder; csrc/stp3_png.hip) on the cases of tests/png_cases.py: handmade streams
whose expected output is their source array, and streams stored in tests/golden/png_cases.npz (scripts/make_golden_png.py) with
the sha256 of Pillow's decode.

Everything is compared EXACTLY: the scanline filters are integer arithmetic modulo 256 with one definition, so every byte of
every case must be equal.  There is no tolerance anywhere in this file."""
import ctypes
import functools
import io
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import png_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCPU = os.path.join(ROOT, 'tests', 'hipcpu')
ORDERS = ('', 'reverse', 'random')
EINVAL, EUNSUP = -10001, -10002


@functools.lru_cache(maxsize=None)
def fixture():
    return PC.load()


@functools.lru_cache(maxsize=None)
def decoder():
    from stp3_amd.datas import PngDecoder
    return PngDecoder(workers=2)


@functools.lru_cache(maxsize=None)
def reference_decode(name):
    """The numpy statement on a case, computed once: (batch, what unfilter returned on the CPU)."""
    batch = decoder().inflate(PC.streams(fixture(), name))
    return batch, decoder().unfilter(batch, 'cpu')


def test_fixture_holds_data_only():
    g = fixture()
    assert os.path.getsize(PC.GOLDEN) <= 200 * 1024
    assert all(v.dtype.kind in 'uUi' for v in g.values())
    assert sorted({k.split('/')[0] for k in g} - {'meta'}) == sorted(list(PC.PILLOW) + list(PC.UNSUPPORTED))
    for name in PC.UNSUPPORTED:                                                   # the stored streams are the helper's
        assert PC.streams(g, name) == [PC.unsupported_stream(name)], name


def chunks(data):
    pos, out = 8, []
    while pos < len(data):
        n = struct.unpack_from('>I', data, pos)[0]
        out.append((data[pos + 4:pos + 8], n))
        pos += 12 + n
    return out


def test_cases_cover_what_they_claim():
    g, dec = fixture(), decoder()
    used = lambda name: set(reference_decode(name)[0].groups[0].rows[0, :, 0].tolist())
    assert [len(PC.source(f'extreme_1x1_c{c}').shape) for c in (1, 2, 3, 4)] == [2, 3, 3, 3]
    assert PC.filters('paeth_first_5x3') == [4, 3, 2, 1, 0]
    for name in ('band_63x5', 'band_64x2', 'band_65x70', 'band_130x33', 'carla_300x400', 'grey_65x257'):
        assert used(name) == {0, 1, 2, 3, 4}, name
    assert PC.HANDMADE['band_63x5']['hw'][0] == PC.BAND - 1 and PC.HANDMADE['band_65x70']['hw'][0] == PC.BAND + 1
    assert PC.HANDMADE['band_130x33']['hw'][0] > 2 * PC.BAND and PC.HANDMADE['band_64x2']['hw'] == (PC.BAND, 2)
    assert PC.PASS < PC.HANDMADE['pass_515x5']['hw'][0] < PC.PASS + PC.BAND < PC.HANDMADE['pass_580x70']['hw'][0] < PC.PASS + 2 * PC.BAND
    assert used('pass_515x5') == used('pass_580x70') == {0, 1, 2, 3, 4}
    assert all(used(f'only_type_{t}') == {t} for t in range(5))
    assert (1 + 257 * 1) % 4 == 2                                                 # the row pitch of grey_65x257
    # hostile values: every tie of the Paeth rule and a = b = c occur, Average meets 9-bit sums, sums wrap
    x = PC.source('hostile_paeth').astype(np.int32)
    a, b, c = x[1:, :-1], x[:-1, 1:], x[:-1, :-1]
    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
    assert ((a == b) & (b == c)).any() and ((pa == pb) & (pa < pc)).any()
    assert ((pb == pc) & (pb < pa) & (b != c)).any() and ((pa == pc) & (pa < pb) & (a != c)).any()
    x = PC.source('hostile_average').astype(np.int32).reshape(24, 96)            # two bytes per pixel
    a, b = x[1:, :-2], x[:-1, 2:]
    assert (a + b >= 256).any()
    rows = reference_decode('hostile_average')[0].groups[0].rows[0].numpy().astype(np.int32)
    assert (rows[1:, 3:] + ((a + b) >> 1) >= 256).any()                           # filtered byte + predictor wraps past 255
    assert PC.filters('independent_runs') == PC.RUNS
    # chunk structure of the stored and the split streams
    assert [k for k, _ in chunks(PC.streams(g, 'three_idat')[0])].count(b'IDAT') == 3
    sizes = [n for k, n in chunks(PC.streams(g, 'three_idat')[0]) if k == b'IDAT']
    assert sizes[0] % 2 == 1 and (sizes[0] + sizes[1]) % 2 == 1
    assert [k for k, _ in chunks(PC.streams(g, 'pillow_large')[0])].count(b'IDAT') >= 2
    names = lambda n: [k for k, _ in chunks(PC.streams(g, n)[0])]
    assert {b'PLTE', b'tRNS'} <= set(names('pillow_palette_trns')) and {b'pHYs', b'tEXt'} <= set(names('pillow_phys_text'))
    assert len(used('pillow_rgb')) >= 3                                           # adaptive filtering
    assert dec.info(PC.streams(g, 'pillow_palette_trns')[0]).colour_type == 3
    assert len(set(PC.CORRUPT)) == 6 and len(set(PC.UNSUPPORTED)) == 5 and len(PC.REFUSED) == 1


@pytest.mark.parametrize('name', PC.SUPPORTED)
def test_numpy_statement_matches(name):
    """unfilter_reference == the source array (handmade) / the stored hash of Pillow's decode (stored); never the fallback."""
    g = fixture()
    batch, got = reference_decode(name)
    assert batch.fallback == {} and len(batch.groups) == 1, name
    assert got.dtype == torch.uint8 and PC.matches(g, name, got.numpy()), name
    want = PC.expected(g, name)
    if want is not None:
        assert np.array_equal(got.numpy(), want), f'{name}: {int((got.numpy() != want).sum())} bytes differ'
    from stp3_amd.datas import PngDecoder
    grp = batch.groups[0]
    flat = PngDecoder.unfilter_reference(grp.rows.numpy(), grp.geometry.bpp)       # arrays in, arrays out
    assert isinstance(flat, np.ndarray) and np.array_equal(flat.reshape(got.shape), got.numpy())


@pytest.mark.parametrize('name', PC.SUPPORTED + list(PC.UNSUPPORTED))
def test_pillow_decodes_the_same(name):
    Image = pytest.importorskip('PIL.Image')
    g = fixture()
    got = [np.asarray(Image.open(io.BytesIO(s))) for s in PC.streams(g, name)]
    assert PC.matches(g, name, got), name
    assert PC.matches(g, name, decoder().reference(PC.streams(g, name)))


def test_info_reports_the_header():
    g, dec = fixture(), decoder()
    f = dec.info(PC.streams(g, 'rgba_70x33')[0])
    assert (f.height, f.width, f.bit_depth, f.colour_type, f.interlace, f.bpp, f.shape) == (70, 33, 8, 6, 0, 4, (70, 33, 4))
    f = dec.info(PC.streams(g, 'grey_65x257')[0])
    assert (f.colour_type, f.bpp, f.shape) == (0, 1, (65, 257))
    f = dec.info(PC.streams(g, 'hostile_average')[0])
    assert (f.colour_type, f.bpp, f.shape) == (4, 2, (24, 48, 2))
    whole = dec.info(PC.write_png(PC.source('three_idat'), PC.filters('three_idat')))
    assert dec.info(PC.streams(g, 'three_idat')[0]).idat == whole.idat           # the payloads, concatenated
    assert dec.info(memoryview(PC.streams(g, 'pillow_phys_text')[0])).shape == (20, 30)


def test_mixed_geometry_is_grouped_and_refilled():
    g, dec = fixture(), decoder()
    names = ('only_type_4', 'only_type_1', 'grey_65x257', 'only_type_3')
    batch = dec.inflate([PC.streams(g, n)[0] for n in names])
    assert [tuple(grp.indices) for grp in batch.groups] == [(0, 1, 3), (2,)] and batch.fallback == {}
    assert tuple(batch.groups[0].rows.shape) == (3, 40, 121) and tuple(batch.groups[1].rows.shape) == (1, 65, 258)
    got = dec.unfilter(batch, 'cpu')
    assert isinstance(got, list) and all(np.array_equal(a.numpy(), PC.source(n)) for a, n in zip(got, names))
    # two cases of one geometry: one group, one stacked tensor; then the batch refilled in place
    first = dec.inflate(PC.streams(g, 'three_images'))
    where = first.groups[0].rows.data_ptr()
    assert np.array_equal(dec.unfilter(first, 'cpu').numpy(), PC.expected(g, 'three_images'))
    second = dec.inflate(PC.streams(g, 'three_images_replay'), out=first)
    assert second.groups[0].rows.data_ptr() == where
    out = torch.full((3, 20, 24, 3), 77, dtype=torch.uint8)
    assert dec.unfilter(second, 'cpu', out=out) is out and np.array_equal(out.numpy(), PC.expected(g, 'three_images_replay'))
    with pytest.raises(ValueError):
        dec.inflate(PC.streams(g, 'only_type_0'), out=first)
    # a group whose images are not consecutive in a call of one shape
    mixed = [PC.streams(g, 'only_type_2')[0], PC.streams(g, 'only_type_0')[0]]
    assert np.array_equal(dec(mixed, 'cpu').numpy(), np.stack([PC.source('only_type_2'), PC.source('only_type_0')]))


@pytest.mark.parametrize('name', PC.CORRUPT)
def test_corrupt_streams_raise(name):
    """Refused on the host, with the image's index; neither the kernel nor Pillow sees them, with or without the fallback."""
    from stp3_amd._lib import Stp3HipError
    from stp3_amd.datas import PngDecoder
    good = PC.streams(fixture(), 'only_type_0')[0]
    for dec in (decoder(), PngDecoder(workers=1, fallback=False)):
        with pytest.raises(Stp3HipError, match='image 1'):
            dec.inflate([good, PC.corrupt(name)])
        with pytest.raises(Stp3HipError, match='image 0'):
            dec([PC.corrupt(name)], 'cpu')


def test_every_truncation_is_refused():
    from stp3_amd._lib import Stp3HipError
    s = PC.streams(fixture(), 'paeth_first_5x3')[0]
    for cut in range(len(s)):
        with pytest.raises(Stp3HipError):
            decoder().inflate([s[:cut]])
    assert decoder().inflate([s]).fallback == {}


def test_only_the_unsupported_streams_take_the_fallback():
    """The cap on the share of cases behind the fallback is zero beyond the named ones: the issue's four and 16-bit grey + alpha."""
    from stp3_amd.datas import PngDecoder, PngUnsupported
    g, dec = fixture(), decoder()
    for name in PC.SUPPORTED:
        assert reference_decode(name)[0].fallback == {}, name
    pytest.importorskip('PIL')
    every = [PC.streams(g, n)[0] for n in PC.SUPPORTED if PC.count(n) == 1] + [PC.streams(g, n)[0] for n in PC.UNSUPPORTED]
    batch = dec.inflate(every)
    assert sorted(batch.fallback) == list(range(len(every) - len(PC.UNSUPPORTED), len(every)))
    for name in PC.UNSUPPORTED:
        s = PC.streams(g, name)
        batch = dec.inflate(s)
        assert list(batch.fallback) == [0] and not batch.groups, name
        assert PC.matches(g, name, dec.unfilter(batch, 'cpu').numpy()), name
        with pytest.raises(PngUnsupported, match='image 1: '):
            PngDecoder(workers=1, fallback=False).inflate(PC.streams(g, 'only_type_0') + s)
    # what Pillow decodes to more than 8 bits per sample is refused whatever `fallback` is, never cut to 8 bits
    for name in PC.REFUSED:
        s = PC.unsupported_stream(name)
        assert dec.reference([s])[0].dtype == np.uint16
        for d in (dec, PngDecoder(workers=1, fallback=False)):
            with pytest.raises(PngUnsupported, match='image 1: 16-bit samples'):
                d(PC.streams(g, 'only_type_0') + [s], 'cpu')
    # a 1-bit image is uint8 0 / 1 in the stacked and in the list form of the result
    alone = dec(PC.streams(g, 'grey_1bit'), 'cpu')
    listed = dec(PC.streams(g, 'grey_1bit') + PC.streams(g, 'only_type_0'), 'cpu')
    assert alone.dtype == listed[0].dtype == torch.uint8 and torch.equal(alone[0], listed[0]) and int(alone.max()) == 1
    apng = PC.streams(g, 'only_type_0')[0]
    at = apng.index(b'IDAT') - 4
    apng = apng[:at] + PC.chunk(b'acTL', struct.pack('>II', 1, 0)) + apng[at:]
    assert list(dec.inflate([apng]).fallback) == [0]
    # a fallback image between kernel images of its shape lands in its slot
    mid = [PC.write_png(np.arange(162, dtype=np.uint8).reshape(6, 9, 3), [4] * 6)]
    assert dec.info(mid[0]).shape == (6, 9, 3)
    got = dec(mid + PC.streams(g, 'rgb_16bit') + mid, 'cpu')
    assert tuple(got.shape) == (3, 6, 9, 3) and PC.matches(g, 'rgb_16bit', got[1:2].numpy()) and torch.equal(got[0], got[2])


def test_c_entry_validates_without_a_gpu():
    from stp3_amd import _lib
    lib = _lib.lib()
    fake = ctypes.c_void_p(64)                                                    # never dereferenced: every call is refused first
    base = dict(rows=fake, n=2, height=30, width=40, bpp=3, out=fake)

    def call(**k):
        a = {**base, **k}
        return lib.stp3_png_unfilter(a['rows'], a['n'], a['height'], a['width'], a['bpp'], a['out'], None)

    for bad in (dict(n=0), dict(height=0), dict(width=-1), dict(bpp=0), dict(bpp=5), dict(rows=None), dict(out=None)):
        assert call(**bad) == EINVAL, bad
    for unsupported in (dict(width=16385), dict(height=20000)):
        assert call(**unsupported) == EUNSUP, unsupported


def test_wrapper_raises():
    from stp3_amd._lib import Stp3HipError
    from stp3_amd.datas import PngDecoder
    g, dec = fixture(), decoder()
    batch = dec.inflate(PC.streams(g, 'only_type_0'))
    with pytest.raises(ValueError):
        dec.unfilter(batch, 'cpu', out=torch.empty(1, 40, 40, 3))                 # not uint8
    with pytest.raises(ValueError):
        dec.unfilter(batch, 'cpu', out=torch.empty(1, 40, 41, 3, dtype=torch.uint8))
    grp = batch.groups[0]
    with pytest.raises(ValueError):
        dec.unfilter_device(grp.geometry, grp.rows[:, :, :-1])
    with pytest.raises(Stp3HipError):
        dec.unfilter_device(grp.geometry, grp.rows)                               # CPU tensors: there is no silent fallback here
    with pytest.raises(ValueError):
        PngDecoder.unfilter_reference(grp.rows, 5)
    with pytest.raises(ValueError):
        PngDecoder.unfilter_reference(grp.rows[:, :, :-1], 3)                     # 119 bytes are no whole number of pixels
    # a filter type above 4 cannot come from inflate; the statement treats it as None, as the kernel does
    rows = np.array([[[9, 1, 2, 3], [1, 4, 5, 6]]], dtype=np.uint8)
    assert PngDecoder.unfilter_reference(rows, 1).tolist() == [[[1, 2, 3], [4, 9, 15]]]


# ---- a CARLA sample from its files' bytes ------------------------------------------------------------------------------
def test_load_carla_sample_from_bytes_on_the_cpu():
    from stp3_amd import carla
    files, arrays, m = PC.carla_files()
    dec = carla.CarlaDecoder(crop=256, bev_crop=200)
    got = carla.load_carla_sample(dec, decoder(), **files, **m, generator=torch.Generator().manual_seed(3), device='cpu')
    want = carla.assemble_carla_sample(dec, *(torch.from_numpy(a) for a in arrays), **m, generator=torch.Generator().manual_seed(3))
    assert PC.sample_difference(got, want) == []
    assert tuple(got['image'].shape) == (2, 4, 3, 256, 256) and tuple(got['segmentation'].shape) == (4, 1, 200, 200)
    # a camera file that is not RGB, a top-down file that is not 2-D: ValueError with the file's index
    grey = PC.write_png(arrays[0][0, 0, :, :, 0].copy(), [0] * 258)
    wrong = dict(files, image_files=[files['image_files'][0], files['image_files'][1][:2] + [grey] + files['image_files'][1][3:]])
    with pytest.raises(ValueError, match='camera file 6'):
        carla.load_carla_sample(dec, decoder(), **wrong, **m, device='cpu')
    wrong = dict(files, hdmap_files=[files['hdmap_files'][0], PC.write_png(arrays[3][0], [0] * 224)])
    with pytest.raises(ValueError, match='hd-map file 1'):
        carla.load_carla_sample(dec, decoder(), **wrong, **m, device='cpu')
    wrong = dict(files, topdown_files=files['topdown_files'][:3] + [files['hdmap_files'][0]])
    with pytest.raises(ValueError, match='top-down file 3'):
        carla.load_carla_sample(dec, decoder(), **wrong, **m, device='cpu')
    wrong = dict(files, depth_files=[files['depth_files'][0][:3], files['depth_files'][1]])
    with pytest.raises(ValueError):
        carla.load_carla_sample(dec, decoder(), **wrong, **m, device='cpu')


# ---- the kernel source on the host ---------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def host_lib(tmp_path_factory):
    sys.path.insert(0, HIPCPU)
    import build as hipcpu_build
    tmp = tmp_path_factory.mktemp('hipcpu_png')
    return tmp, hipcpu_build.build(str(tmp / 'libstp3hip_cpu.so'), sources=[os.path.join(ROOT, 'st-p3_amd', 'csrc', 'stp3_png.hip')])


@pytest.fixture(scope='module', params=ORDERS)
def host_kernel(request, host_lib):
    tmp, lib = host_lib
    env = dict(os.environ)
    env.pop('HIPCPU_ORDER', None)
    if request.param:
        env['HIPCPU_ORDER'] = request.param
    path = str(tmp / f'out_{request.param or "plain"}.npz')
    out = subprocess.run([sys.executable, os.path.join(HIPCPU, 'run_png.py'), lib, path], env=env, capture_output=True,
                         text=True, timeout=3000)
    assert out.returncode == 0 and 'RESULT' in out.stdout, out.stderr[-1500:]
    return request.param or 'plain', dict(np.load(path))


def test_kernel_on_host_matches(host_kernel):
    """The kernel source under three fiber orders, dynamic LDS poisoned: every supported case, the guard ring, the replay."""
    order, out = host_kernel
    g = fixture()
    for name in PC.SUPPORTED:
        assert out[name].dtype == np.uint8 and bool(out[f'{name}/guard']), (order, name)
        want = PC.expected(g, name)
        if want is not None:
            assert out[name].shape == want.shape, (order, name)
            assert np.array_equal(out[name], want), f'{order} order, {name}: {int((out[name] != want).sum())} bytes differ'
        assert PC.matches(g, name, out[name]), (order, name)
    assert np.array_equal(out['replay'], PC.expected(g, 'three_images_replay')), order
