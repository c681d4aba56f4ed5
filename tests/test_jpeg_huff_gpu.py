"""GPU: the device entropy decode of the JPEG decoder (``JpegDecoder(entropy='device')``; csrc/stp3_jpeg_huff.hip) on the cases
of tests/jpeg_huff_cases.py: coefficients and tables against the host decoder (stp3_jpeg_entropy) element for element, decoded
images against Pillow's bytes or their sha256.  Only stored fixtures are read.  Every comparison is exact equality.  The
streams that must be refused here have passed the corruption sweep of tests/test_jpeg_huff_cpu.py first; there is no sweep on
the GPU."""
import functools

import numpy as np
import pytest
import torch

from tests import jpeg_cases as JC
from tests import jpeg_huff_cases as HC

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def fixtures():
    return {'jpeg': JC.load(), 'huff': HC.load()}


@functools.lru_cache(maxsize=None)
def decoders():
    from stp3_amd.datas import JpegDecoder
    return JpegDecoder(workers=2), JpegDecoder(workers=2, entropy='device')


def streams_of(key, name):
    return (JC if key == 'jpeg' else HC).streams(fixtures()[key], name)


@pytest.mark.parametrize('key,name', HC.all_cases())
def test_device_decode_equals_the_host_decoder(key, name):
    host, dev = decoders()
    streams = streams_of(key, name)
    want = host.entropy(streams)
    groups, _ = dev.entropy_device(streams, 'cuda')
    assert dev.last_stats == {'device': len(streams), 'host': 0, 'pillow': 0}, dev.last_stats
    assert [(g.geometry, g.indices) for g in groups] == want.layout()
    for g, w in zip(groups, want.groups):
        assert g.coef.is_cuda and g.coef.dtype == torch.int16
        differ = int((g.coef.cpu() != w.coef).sum())
        print(f'{name}: {differ} of {w.coef.numel()} coefficients differ')
        assert differ == 0 and torch.equal(g.quant.cpu(), w.quant), name
    got = dev(streams, 'cuda')
    assert dev.last_stats == {'device': len(streams), 'host': 0, 'pillow': 0}, dev.last_stats
    assert got.is_cuda and got.dtype == torch.uint8
    if key == 'jpeg':
        assert np.array_equal(got.cpu().numpy(), JC.expected(fixtures()['jpeg'], name)), name
    else:
        assert [HC.digest(im) for im in got.cpu().numpy()] == HC.expected_digests(fixtures()['huff'], name), name


def test_without_cross_workgroup_rounds_the_host_decodes():
    from stp3_amd import _lib
    from stp3_amd.datas import JpegDecoder
    dec = JpegDecoder(workers=2, entropy='device', sync_rounds=0)
    streams = streams_of('huff', 'multi_wg')
    batch = dec.prepare(streams)
    grp = batch.groups[0]
    coef = torch.empty(1, grp.descs.numpy().view(np.int32)[0, 12], dtype=torch.int16, device='cuda')
    status = torch.zeros(1, dtype=torch.int32, device='cuda')
    dec.entropy_device_launch(grp, grp.scans.cuda(), grp.descs.cuda(), coef, status)
    assert status.cpu().tolist() == [_lib.STP3_JPEG_NOT_CONVERGED]
    got = dec(streams, 'cuda')
    assert dec.last_stats == {'device': 0, 'host': 1, 'pillow': 0}
    assert [HC.digest(im) for im in got.cpu().numpy()] == HC.expected_digests(fixtures()['huff'], 'multi_wg')
    # one workgroup needs no further round
    dec(streams_of('huff', 'wg_sync'), 'cuda')
    assert dec.last_stats == {'device': 1, 'host': 0, 'pillow': 0}


def test_held_buffers_are_refilled():
    """Static device buffers, decoded, refilled with a second batch of the same layout, decoded again: the coefficients are
    the second batch's in every element (the clear of `coef` is part of the call)."""
    host, dev = decoders()
    names = ['s420_32x48_n3', 's420_32x48_n3_replay']
    batches = [dev.prepare(streams_of('jpeg', n)) for n in names]
    if batches[1].groups[0].stride > batches[0].groups[0].stride:
        names.reverse()
        batches.reverse()
    batch, grp = batches[0], batches[0].groups[0]
    scans, descs = grp.scans.cuda(), grp.descs.cuda()
    coef = torch.full((3, 32 * 48 * 3 // 2), 0x5A5A, dtype=torch.int16, device='cuda')
    status = torch.full((3,), -1, dtype=torch.int32, device='cuda')
    for name in names:
        again = dev.prepare(streams_of('jpeg', name), out=batch)
        assert again.groups[0].scans.data_ptr() == grp.scans.data_ptr()
        scans.copy_(grp.scans)
        descs.copy_(grp.descs)
        dev.entropy_device_launch(grp, scans, descs, coef, status)
        assert status.cpu().tolist() == [0, 0, 0], name
        want = host.entropy(streams_of('jpeg', name)).groups[0]
        assert torch.equal(coef.cpu(), want.coef) and torch.equal(grp.quant, want.quant), name


def test_streams_that_must_be_refused():
    from stp3_amd._lib import Stp3HipError
    host, dev = decoders()
    crafted = JC.crafted_refused()
    s = streams_of('huff', 'wg_sync')[0]
    refused = {'dc_times_quant': crafted['dc_times_quant'], 'ac_times_quant': crafted['ac_times_quant'],
               'cut_at_the_first_edge': s[:HC.scan_offset(s) + HC.S]}
    for name, stream in refused.items():
        with pytest.raises(Stp3HipError, match='image 0') as in_host_mode:
            host([stream], 'cuda')
        with pytest.raises(Stp3HipError, match='image 0') as in_device_mode:
            dev([stream], 'cuda')
        assert str(in_device_mode.value) == str(in_host_mode.value), name
    # ... and a good image beside a bad one: the bad one's index
    with pytest.raises(Stp3HipError, match='image 1'):
        dev([s, refused['cut_at_the_first_edge']], 'cuda')


def test_device_mode_feeds_the_image_preprocessor():
    from stp3_amd.datas import ImagePreprocessor
    host, dev = decoders()
    streams = streams_of('huff', 'multi_wg')
    prep = ImagePreprocessor(resize_dims=(240, 160), crop=(8, 16, 232, 144), source_hw=(320, 480))
    got = prep(dev(streams, 'cuda'))
    assert dev.last_stats['device'] == 1
    want = prep(host(streams, 'cuda'))
    assert tuple(got.shape) == (1, 3, 128, 224) and torch.equal(got, want)
