"""CPU: the JPEG decoder (stp3_amd.datas.JpegDecoder; csrc/stp3_jpeg_entropy.h, csrc/stp3_jpeg.hip) against Pillow's decode
of the streams stored in tests/golden/jpeg_cases.npz (scripts/make_golden_jpeg.py) on the cases of tests/jpeg_cases.py.

Everything is compared EXACTLY: libjpeg's slow-integer IDCT, fancy up-sampling and table colour conversion are integer
arithmetic, so every byte of every case must equal Pillow's.  There is no tolerance anywhere in this file."""
import ctypes
import functools
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import jpeg_cases as JC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCPU = os.path.join(ROOT, 'tests', 'hipcpu')
ORDERS = ('', 'reverse', 'random')
EINVAL, EUNSUP = -10001, -10002


@functools.lru_cache(maxsize=None)
def fixture():
    return JC.load()


@functools.lru_cache(maxsize=None)
def decoder():
    from stp3_amd.datas import JpegDecoder
    return JpegDecoder(workers=2)


def raw_entropy(data, capacity=None, guard=64):
    """stp3_jpeg_entropy on `data` with guard words around both buffers: (return code, header, coefficients, guards intact)."""
    from stp3_amd import _lib
    lib = _lib.lib()
    h = _lib.JpegHeader()
    rc = lib.stp3_jpeg_info(data, len(data), ctypes.byref(h))
    n = capacity if capacity is not None else (h.coef_count if rc == 0 else 4096)
    coef = np.full(n + 2 * guard, 0x5A5A, dtype=np.int16)
    quant = np.full(192 + 2 * guard, 0x5A5A, dtype=np.uint16)
    rc2 = lib.stp3_jpeg_entropy(data, len(data), coef[guard:].ctypes.data, n, quant[guard:].ctypes.data, ctypes.byref(h))
    intact = ((coef[:guard] == 0x5A5A).all() and (coef[guard + n:] == 0x5A5A).all() and (quant[:guard] == 0x5A5A).all() and
              (quant[guard + 192:] == 0x5A5A).all())
    return rc, rc2, h, coef[guard:guard + n], bool(intact)


def test_fixture_holds_data_only():
    g = fixture()
    assert os.path.getsize(JC.GOLDEN) <= 200 * 1024
    assert all(v.dtype.kind in 'uU' for v in g.values())
    assert sorted({k.split('/')[0] for k in g} - {'meta'}) == sorted(JC.CASES)
    for name, c in JC.CASES.items():
        assert JC.expected(g, name).shape == (c.get('images', 1),) + tuple(c['hw']) + (3,)


def test_cases_cover_what_they_claim():
    g, dec = fixture(), decoder()
    layer = {name: dec.info(JC.streams(g, name)[0]) for name in JC.SUPPORTED}
    assert (layer['s444_8x8'].mcus_x, layer['s444_8x8'].mcus_y, layer['s444_8x8'].hs) == (1, 1, 1)
    assert layer['s420_16x16'].blocks == ((2, 2), (1, 1), (1, 1))
    assert layer['s420_23x37'].width % 2 == 1 and -(-layer['s420_23x37'].width // 2) % 2 == 1 and layer['s420_23x37'].height % 2 == 1
    assert (layer['s422_40x17'].hs, layer['s422_40x17'].vs, layer['s422_40x17'].width % 2) == (2, 1, 1)
    assert layer['s420_48x64_rst_row'].restart_interval == layer['s420_48x64_rst_row'].mcus_x == 4
    assert layer['s420_48x64_rst_3'].restart_interval == 3                      # intervals that straddle MCU rows
    for name in ('s420_48x64_rst_row', 's420_48x64_rst_3'):
        assert JC.streams(g, name)[0].count(b'\xff\xd1') >= 1, name              # a second restart marker is in the stream
    assert layer['grey_13x9'].components == 1
    assert -(-layer['s420_16x4'].width // 2) == 2 and -(-layer['s422_9x3'].width // 2) == 2
    # per-image tables in one launch; quantisers 1 and 255-class; custom Huffman tables
    b = dec.entropy(JC.streams(g, 's420_32x48_n3'))
    q = b.groups[0].quant.numpy().view(np.uint16)
    assert len({q[k].tobytes() for k in range(3)}) == 3
    assert (dec.entropy(JC.streams(g, 's420_40x40_q100')).groups[0].quant == 1).all()
    assert dec.entropy(JC.streams(g, 's420_40x40_q5')).groups[0].quant.numpy().view(np.uint16).max() >= 200
    dht = lambda s: s[s.index(b'\xff\xc4'):s.index(b'\xff\xda')]
    assert dht(JC.streams(g, 's420_40x40_opt')[0]) != dht(JC.streams(g, 's420_40x40_q5')[0])
    # the halo between workgroups and a last partial strip; the strip the kernel reports is the one the case assumes
    from stp3_amd import _lib
    assert _lib.lib().stp3_jpeg_strip_rows(2) == JC.STRIP_420 and _lib.lib().stp3_jpeg_strip_rows(1) == 16
    assert layer['s420_strips'].height == 3 * JC.STRIP_420 + 5 and layer['s444_strips'].height == 2 * 16 + 3
    # the range limit is reached: saturated bytes in the expected output of the hard-edged cases
    assert (JC.expected(g, 's420_40x40_q5') == 255).any() and (JC.expected(g, 's420_40x40_q5') == 0).any()


@pytest.mark.parametrize('name', sorted(JC.CASES))
def test_stored_bytes_are_pillows_decode(name):
    Image = pytest.importorskip('PIL.Image')
    g = fixture()
    for k, s in enumerate(JC.streams(g, name)):
        want = np.asarray(Image.open(io.BytesIO(s)).convert('RGB'))
        assert np.array_equal(want, g[f'{name}/{k}/rgb']), (name, k)
    assert torch.equal(decoder().reference(JC.streams(g, name)), torch.from_numpy(JC.expected(g, name)))


@pytest.mark.parametrize('name', JC.SUPPORTED)
def test_numpy_statements_match_pillow(name):
    g, dec = fixture(), decoder()
    batch = dec.entropy(JC.streams(g, name))
    assert not batch.fallback and len(batch.groups) == 1
    got = dec.reconstruct_reference(batch)
    assert got.dtype == torch.uint8
    want = JC.expected(g, name)
    assert np.array_equal(got.numpy(), want), f'{name}: {int((got.numpy() != want).sum())} bytes differ'
    assert torch.equal(dec(JC.streams(g, name), 'cpu'), got)                     # CPU tensors take that route


@pytest.mark.parametrize('name', JC.SUPPORTED)
def test_info_reports_pillows_geometry(name):
    Image = pytest.importorskip('PIL.Image')
    g, dec = fixture(), decoder()
    for s in JC.streams(g, name):
        im = Image.open(io.BytesIO(s))
        f = dec.info(s)
        assert (f.width, f.height) == im.size and f.components == len(im.layer)
        if f.components == 3:
            assert [(h, v) for _, h, v, _ in im.layer] == [(f.hs, f.vs), (1, 1), (1, 1)]
        assert f.coef_count == sum(by * bx for by, bx in f.blocks) * 64


@pytest.mark.parametrize('name', JC.UNSUPPORTED)
def test_unsupported_streams_fall_back_or_raise(name):
    from stp3_amd.datas import JpegDecoder, JpegUnsupported
    g = fixture()
    s = JC.streams(g, name)
    rc, rc2, _, coef, intact = raw_entropy(s[0])
    assert rc == EUNSUP and rc2 == EUNSUP and intact and (coef == 0x5A5A).all()     # never a partial result
    with pytest.raises(JpegUnsupported, match='image 1: '):
        JpegDecoder(workers=1, fallback=False).entropy(JC.streams(g, 's420_16x16') + s)
    pytest.importorskip('PIL')
    batch = decoder().entropy(s)
    assert list(batch.fallback) == [0] and not batch.groups
    assert np.array_equal(decoder().reconstruct(batch, 'cpu').numpy(), JC.expected(g, name))


def test_mixed_geometry_is_grouped():
    pytest.importorskip('PIL')
    g, dec = fixture(), decoder()
    names = ('s420_40x40_q5', 's420_40x40_opt', 'grey_13x9', 's420_40x40_q100')
    batch = dec.entropy([JC.streams(g, n)[0] for n in names])
    assert [tuple(grp.indices) for grp in batch.groups] == [(0, 1, 3), (2,)]
    got = dec.reconstruct(batch, 'cpu')
    assert isinstance(got, list) and all(np.array_equal(a.numpy(), JC.expected(g, n)[0]) for a, n in zip(got, names))
    # streams of two cases with one geometry: one group, one stacked tensor
    names = ('s420_48x64_rst_row', 's420_48x64_rst_3')
    same = dec([JC.streams(g, n)[0] for n in names], 'cpu')
    assert tuple(same.shape) == (2, 48, 64, 3) and all(np.array_equal(same[i].numpy(), JC.expected(g, n)[0]) for i, n in enumerate(names))


def test_a_batch_is_refilled_in_place():
    g, dec = fixture(), decoder()
    first = dec.entropy(JC.streams(g, 's420_32x48_n3'))
    where = first.groups[0].coef.data_ptr()
    second = dec.entropy(JC.streams(g, 's420_32x48_n3_replay'), out=first)
    assert second.groups[0].coef.data_ptr() == where
    assert np.array_equal(dec.reconstruct_reference(second).numpy(), JC.expected(g, 's420_32x48_n3_replay'))
    with pytest.raises(ValueError):
        dec.entropy(JC.streams(g, 's420_16x16'), out=first)


# ---- error paths: STP3_EINVAL, nothing written outside the buffers -------------------------------------------------------
def test_every_truncation_is_refused():
    s = JC.streams(fixture(), JC.TRUNCATE[0])[0]
    for cut in range(len(s)):
        rc, rc2, _, _, intact = raw_entropy(s[:cut])
        assert rc2 == EINVAL and intact, (cut, rc, rc2)
    assert raw_entropy(s)[1] == 0


def scan_offset(s):
    at = s.index(b'\xff\xda')
    return at + 2 + ((s[at + 2] << 8) | s[at + 3])


def with_tables(s, counts, symbols, table):
    """`s` with the Huffman table `table` (Tc << 4 | Th) redefined just in front of the scan header."""
    at = s.index(b'\xff\xda')
    seg = bytes([table]) + bytes(counts) + bytes(symbols)
    return s[:at] + b'\xff\xc4' + (len(seg) + 2).to_bytes(2, 'big') + seg + s[at:]


def test_a_code_no_table_assigns_is_refused():
    s = JC.streams(fixture(), 'grey_13x9')[0]
    # DC table: the single code '0' (category 0); the scan starts with a 1 bit
    bad = with_tables(s, [1] + [0] * 15, [0], 0x00)
    bad = bad[:scan_offset(bad)] + b'\xf0' * 8 + b'\xff\xd9'
    rc, rc2, _, _, intact = raw_entropy(bad)
    assert (rc, rc2) == (0, EINVAL) and intact
    with pytest.raises(Exception, match='image 0'):
        decoder().entropy([bad])


def test_a_run_past_coefficient_63_is_refused():
    s = JC.streams(fixture(), 'grey_13x9')[0]
    # DC: '0' = category 0.  AC: '0' = run 15 / size 1 (0xF1): five of them reach index 80
    bad = with_tables(with_tables(s, [1] + [0] * 15, [0], 0x00), [1] + [0] * 15, [0xF1], 0x10)
    bad = bad[:scan_offset(bad)] + b'\x00' * 16 + b'\xff\xd9'
    rc, rc2, _, _, intact = raw_entropy(bad)
    assert (rc, rc2) == (0, EINVAL) and intact
    # ... and sixteen-zero runs (0xF0) past the end of the block
    bad = with_tables(with_tables(s, [1] + [0] * 15, [0], 0x00), [1] + [0] * 15, [0xF0], 0x10)
    bad = bad[:scan_offset(bad)] + b'\x00' * 16 + b'\xff\xd9'
    assert raw_entropy(bad)[1] == EINVAL


def test_a_scan_naming_a_missing_table_is_refused():
    s = bytearray(JC.streams(fixture(), 'grey_13x9')[0])
    at = s.index(b'\xff\xda')
    assert s[at + 4] == 1 and s[at + 6] == 0x00                                   # one component, tables 0 / 0
    s[at + 6] = 0x22                                                              # tables 2 / 2: never defined
    rc, rc2, _, _, intact = raw_entropy(bytes(s))
    assert rc == EINVAL and rc2 == EINVAL and intact


@pytest.mark.parametrize('name', sorted(JC.crafted_refused()))
def test_coefficients_no_encoder_writes_are_refused(name):
    """Valid syntax, illegal values: a DC predictor walked out of 16 (and, unchecked, of 32) bits over many blocks, and
    coefficients whose dequantised value leaves 16 bits.  STP3_EINVAL, never STP3_OK with wrapped coefficients."""
    s = JC.crafted_refused()[name]
    rc, rc2, _, _, intact = raw_entropy(s)
    assert (rc, rc2) == (0, EINVAL) and intact, name
    with pytest.raises(Exception, match='image 0'):
        decoder().entropy([s])


def test_legal_extremes_still_decode():
    """DC differences of +1016 per block at quantiser 1 (the running DC reaches 4064: far beyond what samples can hold, inside
    16 bits): decoded, and the range limit gives Pillow's bytes."""
    s = JC.crafted_grey(16, 16, 1, 10, '1111111000', 0x00, '')
    rc, rc2, h, coef, intact = raw_entropy(s)
    assert (rc, rc2) == (0, 0) and intact and [int(coef[64 * b]) for b in range(4)] == [1016, 2032, 3048, 4064]
    got = decoder().reconstruct_reference(decoder().entropy([s])).numpy()
    assert (got[0, :8, :8] == 255).all()                                          # (1016 * 4 + 16 >> 5) + 128 = 255
    Image = pytest.importorskip('PIL.Image')
    assert np.array_equal(got[0], np.asarray(Image.open(io.BytesIO(s)).convert('RGB')))


def test_bytes_in_front_of_a_marker_are_skipped():
    """Padding or junk between the entropy data and EOI / RSTn: libjpeg skips it with a warning, so does the decoder; the
    picture is the fixture's."""
    g, dec = fixture(), decoder()
    for name in ('s420_16x16', 's420_48x64_rst_row'):
        s = JC.streams(g, name)[0]
        assert s.endswith(b'\xff\xd9')
        junk = s[:-2] + b'\x00\x12\x34\xff\x00\x56' + b'\xff\xd9'
        if name.endswith('rst_row'):
            at = junk.index(b'\xff\xd0')
            junk = junk[:at] + b'\x77\x00' + junk[at:]
        assert np.array_equal(dec.reconstruct_reference(dec.entropy([junk])).numpy(), JC.expected(g, name)), name
        assert raw_entropy(s[:-2] + b'\x00\x12\x34')[1] == EINVAL                 # ... but EOI itself must come


def test_a_buffer_too_small_is_refused_untouched():
    s = JC.streams(fixture(), 's420_16x16')[0]
    rc, rc2, h, coef, intact = raw_entropy(s, capacity=383)
    assert rc == 0 and h.coef_count == 384 and rc2 == EINVAL and intact and (coef == 0x5A5A).all()


def test_c_entry_validates_without_a_gpu():
    from stp3_amd import _lib
    lib = _lib.lib()
    fake = ctypes.c_void_p(64)                                                    # never dereferenced: every call is refused first
    base = dict(N=2, width=64, height=48, components=3, hs=2, vs=2)

    def call(coef=fake, quant=fake, out=fake, **k):
        return lib.stp3_jpeg_reconstruct(ctypes.byref(_lib.JpegDims(**{**base, **k})), coef, quant, out, None)

    for bad in (dict(N=0), dict(width=0), dict(height=-1), dict(components=2), dict(components=4), dict(hs=4, vs=1), dict(hs=1, vs=2),
                dict(components=1), dict(hs=3), dict(coef=None), dict(quant=None), dict(out=None)):
        assert call(**bad) == EINVAL, bad
    for unsupported in (dict(N=70000), dict(width=20000), dict(width=4000)):      # (LDS: a strip 4 000 pixels wide)
        assert call(**unsupported) == EUNSUP, unsupported
    assert lib.stp3_jpeg_reconstruct(None, fake, fake, fake, None) == EINVAL
    h = _lib.JpegHeader()
    assert lib.stp3_jpeg_info(None, 0, ctypes.byref(h)) == EINVAL and lib.stp3_jpeg_info(b'\xff\xd8', 2, None) == EINVAL


def test_wrapper_raises():
    g, dec = fixture(), decoder()
    batch = dec.entropy(JC.streams(g, 's420_16x16'))
    with pytest.raises(ValueError):
        dec.reconstruct(batch, 'cpu', out=torch.empty(1, 16, 16, 3))             # not uint8
    with pytest.raises(ValueError):
        dec.reconstruct(batch, 'cpu', out=torch.empty(1, 16, 17, 3, dtype=torch.uint8))
    grp = batch.groups[0]
    with pytest.raises(ValueError):
        dec.reconstruct_device(grp.geometry, grp.coef[:, :-1], grp.quant)
    from stp3_amd._lib import Stp3HipError
    with pytest.raises(Stp3HipError):
        dec.reconstruct_device(grp.geometry, grp.coef, grp.quant)                # CPU tensors: there is no silent fallback here


# ---- the kernel source on the host ---------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def host_lib(tmp_path_factory):
    sys.path.insert(0, HIPCPU)
    import build as hipcpu_build
    tmp = tmp_path_factory.mktemp('hipcpu_jpeg')
    return tmp, hipcpu_build.build(str(tmp / 'libstp3hip_cpu.so'), sources=[os.path.join(ROOT, 'st-p3_amd', 'csrc', 'stp3_jpeg.hip')])


@pytest.fixture(scope='module', params=ORDERS)
def host_kernel(request, host_lib):
    tmp, lib = host_lib
    env = dict(os.environ)
    env.pop('HIPCPU_ORDER', None)
    if request.param:
        env['HIPCPU_ORDER'] = request.param
    path = str(tmp / f'out_{request.param or "plain"}.npz')
    out = subprocess.run([sys.executable, os.path.join(HIPCPU, 'run_jpeg.py'), lib, path], env=env, capture_output=True,
                         text=True, timeout=3000)
    assert out.returncode == 0 and 'RESULT' in out.stdout, out.stderr[-1500:]
    return request.param or 'plain', dict(np.load(path))


def test_kernel_on_host_matches_pillow(host_kernel):
    """The kernel source under three fiber orders, dynamic LDS poisoned: every case, the fallback ones included."""
    order, out = host_kernel
    g = fixture()
    for name in JC.CASES:
        want = JC.expected(g, name)
        assert out[name].shape == want.shape and out[name].dtype == np.uint8, (order, name)
        assert np.array_equal(out[name], want), f'{order} order, {name}: {int((out[name] != want).sum())} bytes differ'
    assert np.array_equal(out['replay'], JC.expected(g, 's420_32x48_n3_replay')), order
