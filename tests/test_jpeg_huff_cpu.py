"""CPU: the device entropy decode of the JPEG decoder (``JpegDecoder(entropy='device')``; csrc/stp3_jpeg_entropy.h
stp3_jpeg_scan_prepare, csrc/stp3_jpeg_huff.hip) through the host stand-in of the HIP runtime, under the fiber orders
tests/test_jpeg_cpu.py uses, on the cases of tests/jpeg_huff_cases.py.

The host decoder (stp3_jpeg_entropy) is the statement of the result: coefficients and tables are compared with it element for
element, decoded images with Pillow's bytes (tests/golden/jpeg_cases.npz) or their sha256 (tests/golden/jpeg_huff_cases.npz).
Every comparison is exact; there is no tolerance in this file."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import jpeg_cases as JC
from tests import jpeg_huff_cases as HC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCPU = os.path.join(ROOT, 'tests', 'hipcpu')
ORDERS = ('', 'reverse', 'random')
EINVAL = -10001


@functools.lru_cache(maxsize=None)
def fixtures():
    return {'jpeg': JC.load(), 'huff': HC.load()}


def test_fixture_holds_data_only_and_hits_what_it_claims():
    g = fixtures()['huff']                                                       # (HC.load asserts subsequences, workgroups, stuffing)
    assert os.path.getsize(HC.GOLDEN) <= 600 * 1024
    assert all(v.dtype.kind in 'uU' for v in g.values())
    assert sorted({k.split('/')[0] for k in g} - {'meta'}) == sorted(HC.CASES)
    from stp3_amd import _lib
    assert (_lib.JPEG_SUB_BYTES, _lib.JPEG_SUB_THREADS) == (HC.S, HC.G)
    assert len(HC.streams(g, 'multi_wg')[0]) > 3 * HC.S * HC.G
    tables = {s[s.index(b'\xff\xc4'):s.index(b'\xff\xda')] for s in HC.streams(g, 'n3_mixed')}
    assert len(tables) >= 2                                                      # per-image Huffman tables in one launch


def test_stored_digests_are_pillows_decode():
    Image = pytest.importorskip('PIL.Image')
    import io
    g = fixtures()['huff']
    for name in HC.CASES:
        for s, want in zip(HC.streams(g, name), HC.expected_digests(g, name)):
            assert HC.digest(np.asarray(Image.open(io.BytesIO(s)).convert('RGB'))) == want, name


def test_mode_is_an_option_and_the_default_stays():
    from stp3_amd.datas import JpegDecoder
    assert JpegDecoder().entropy_mode == 'host'
    with pytest.raises(ValueError):
        JpegDecoder(entropy='gpu')
    with pytest.raises(ValueError):
        JpegDecoder(entropy='device', sync_rounds=-1)
    # on a CPU device the mode is the host decoder
    g = fixtures()['huff']
    dec = JpegDecoder(workers=1, entropy='device')
    got = dec(HC.streams(g, 'wg_sync'), 'cpu')
    assert HC.digest(got.numpy()[0]) == HC.expected_digests(g, 'wg_sync')[0]
    assert dec.last_stats == {'device': 0, 'host': 1, 'pillow': 0}
    from stp3_amd._lib import Stp3HipError
    with pytest.raises(Stp3HipError):
        dec.entropy_device(HC.streams(g, 'one_sub'), 'cpu')                      # no silent fallback


def test_prepare_routes_streams():
    """Unsupported streams to Pillow, irregular ones (junk in front of a marker is data to a walk that decodes nothing, fill
    bytes are not) to the host decoder, the rest to the device; a batch is refilled in place."""
    pytest.importorskip('PIL')
    from stp3_amd.datas import JpegDecoder
    g = fixtures()
    dec = JpegDecoder(workers=2, entropy='device')
    s = HC.streams(g['huff'], 'n3_mixed')
    fill = s[1][:-2] + b'\xff\xff\xd9'
    batch = dec.prepare([s[0], JC.streams(g['jpeg'], 'progressive')[0], fill, s[2]])
    assert list(batch.fallback) == [1] and batch.layout()[0][1] == (0, 2, 3) and batch.groups[0].host == [1]
    words = batch.groups[0].descs.numpy().view(np.int32)
    assert words[0, 1] == 1 and words[2, 1] == 3 and words[1, 0] == 0           # segments; the irregular one has no descriptor
    where = batch.groups[0].scans.data_ptr()
    again = dec.prepare([s[2], JC.streams(g['jpeg'], 'progressive')[0], s[1], s[0]], out=batch)
    assert again.groups[0].scans.data_ptr() == where and again.groups[0].host == []
    with pytest.raises(ValueError):
        dec.prepare(s, out=batch)


def test_c_entries_validate_without_a_gpu():
    import ctypes
    from stp3_amd import _lib
    lib = _lib.lib()
    fake, n = ctypes.c_void_p(64), ctypes.c_size_t()
    base = dict(N=2, width=64, height=48, components=3, hs=2, vs=2, scan_stride=1024, max_subs=4, max_segs=1)
    dims = lambda **k: ctypes.byref(_lib.JpegHuffDims(**{**base, **k}))
    assert lib.stp3_jpeg_entropy_workspace_bytes(dims(), 4, ctypes.byref(n)) == 0 and n.value > 0
    for bad in (dict(N=0), dict(components=2), dict(hs=3), dict(scan_stride=0), dict(scan_stride=1022), dict(max_subs=0), dict(max_segs=0)):
        assert lib.stp3_jpeg_entropy_workspace_bytes(dims(**bad), 4, ctypes.byref(n)) == EINVAL, bad
        assert lib.stp3_jpeg_entropy_device(dims(**bad), fake, fake, fake, fake, fake, 1 << 20, 4, None) == EINVAL, bad
    for rounds in (-1, 65):
        assert lib.stp3_jpeg_entropy_workspace_bytes(dims(), rounds, ctypes.byref(n)) == EINVAL
    assert lib.stp3_jpeg_entropy_device(dims(), fake, fake, fake, fake, fake, 16, 4, None) == -10003      # STP3_ENOSPACE
    assert lib.stp3_jpeg_entropy_device(dims(), None, fake, fake, fake, fake, 1 << 20, 4, None) == EINVAL
    h, d = _lib.JpegHeader(), _lib.JpegScanDesc()
    s = HC.streams(fixtures()['huff'], 'one_sub')[0]
    assert lib.stp3_jpeg_info(s, len(s), ctypes.byref(h)) == 0
    need = lib.stp3_jpeg_scan_bytes(ctypes.byref(h), len(s))
    buf, q = ctypes.create_string_buffer(need), ctypes.create_string_buffer(384)
    assert lib.stp3_jpeg_scan_prepare(s, len(s), buf, need, ctypes.byref(d), q) == 0 and d.used_bytes <= need and d.nsub == 1
    assert lib.stp3_jpeg_scan_prepare(s, len(s), buf, d.used_bytes - 1, ctypes.byref(d), q) == EINVAL
    assert lib.stp3_jpeg_scan_prepare(s, len(s), None, need, ctypes.byref(d), q) == EINVAL


# ---- the kernel source on the host -------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def host_lib(tmp_path_factory):
    sys.path.insert(0, HIPCPU)
    import build as hipcpu_build
    tmp = tmp_path_factory.mktemp('hipcpu_jpeg_huff')
    csrc = os.path.join(ROOT, 'st-p3_amd', 'csrc')
    return tmp, hipcpu_build.build(str(tmp / 'libstp3hip_cpu.so'), sources=[os.path.join(csrc, 'stp3_jpeg.hip'),
                                                                            os.path.join(csrc, 'stp3_jpeg_huff.hip')])


@pytest.fixture(scope='module', params=ORDERS)
def host_run(request, host_lib):
    tmp, lib = host_lib
    env = dict(os.environ)
    env.pop('HIPCPU_ORDER', None)
    if request.param:
        env['HIPCPU_ORDER'] = request.param
    path = str(tmp / f'out_{request.param or "plain"}.npz')
    out = subprocess.run([sys.executable, os.path.join(HIPCPU, 'run_jpeg_huff.py'), lib, path], env=env, capture_output=True, text=True,
                         timeout=3000)
    assert out.returncode == 0 and 'RESULT' in out.stdout, out.stderr[-1500:]
    data = dict(np.load(path))
    return request.param or 'plain', data, json.loads(str(data['report']))


def test_device_decode_equals_the_host_decoder(host_run):
    """Coefficients and tables element for element (padding blocks included), through the wrapper and on buffers of exactly
    the announced sizes; every image taken by the device; the guards around every buffer intact."""
    order, out, report = host_run
    for _, name in HC.all_cases():
        images = (JC.CASES if name in JC.CASES else HC.CASES)[name].get('images', 1)
        for what in ('coef_differ', 'quant_differ', 'raw_differ'):
            assert int(out[f'{name}/{what}']) == 0, (order, name, what, int(out[f'{name}/{what}']))
        assert report['status'][name] == [[0, 0]] * images, (order, name, report['status'][name])
        for key in (name, name + '/entropy'):
            assert report['stats'][key] == {'device': images, 'host': 0, 'pillow': 0}, (order, key, report['stats'][key])
        assert all(report['guards'][name]), (order, name)


def test_decoded_images_are_pillows(host_run):
    order, out, _ = host_run
    g = fixtures()
    for name in JC.SUPPORTED:
        assert np.array_equal(out[f'{name}/rgb'], JC.expected(g['jpeg'], name)), (order, name)
    for name in HC.CASES:
        assert [HC.digest(im) for im in out[f'{name}/rgb']] == HC.expected_digests(g['huff'], name), (order, name)


def test_without_cross_workgroup_rounds_the_host_decodes(host_run):
    order, out, report = host_run
    assert report['status']['multi_wg/rounds0'] == report['codes']['not_converged'], order
    assert report['stats']['multi_wg/rounds0'] == {'device': 0, 'host': 1, 'pillow': 0}, order
    assert [HC.digest(im) for im in out['multi_wg/rounds0/rgb']] == HC.expected_digests(fixtures()['huff'], 'multi_wg'), order
    assert report['status']['wg_sync/rounds0'] == 0, order                       # one workgroup needs none


def test_corruption_sweep_ends_as_the_host_decoder_ends(host_run):
    """Every truncation of wg_sync at a subsequence edge +- 1 byte and 300 seeded single-byte corruptions of wg_sync and
    wg_sync_rst: the same bytes, or an exception of the same type with the same image index and text."""
    order, _, report = host_run
    sweep = report['sweep']
    assert len(sweep) >= 2 * HC.CORRUPTIONS + 3 * 60
    for name, r in sweep.items():
        assert r['host'] == r['device'], (order, name, r)
        assert r['guards'], (order, name)
        if r['host'][0] == 'raised':
            assert 'image 0' in r['host'][2], (order, name, r)
    cuts = [r for name, r in sweep.items() if name.startswith('cut/')]
    assert cuts and all(r['host'][0] == 'raised' for r in cuts), order
    # the sweep is not void: streams the device took and decoded, streams it reported, streams prepare called irregular
    decoded = [r for r in sweep.values() if r['host'][0] == 'ok']
    assert sum(r['stats']['device'] == 1 for r in decoded) >= 50, order
    assert sum(r['status'] is not None and r['status'][1] == EINVAL for r in sweep.values()) >= 50, order
    assert sum(r['status'] is not None and r['status'][0] == report['codes']['irregular'] for r in sweep.values()) >= 20, order


def test_crafted_streams_are_refused(host_run):
    order, _, report = host_run
    assert sorted(report['crafted']) == sorted(JC.crafted_refused())
    for name, r in report['crafted'].items():
        assert r['host'][0] == 'raised' and r['device'] == r['host'] and 'image 0' in r['device'][2], (order, name, r)
        assert r['status'] == [0, EINVAL] and r['guards'], (order, name, r)
