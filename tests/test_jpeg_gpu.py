"""GPU: the JPEG decoder (stp3_amd.datas.JpegDecoder; csrc/stp3_jpeg.hip: stp3_jpeg_reconstruct) against Pillow's decode
recorded in tests/golden/jpeg_cases.npz on the cases of tests/jpeg_cases.py.  Only the stored fixture is read; the streams
behind the fallback are decoded by Pillow inside the call, which is the fallback -- without Pillow those tests FAIL, they do
not skip.  Every comparison is exact equality of every byte."""
import functools

import numpy as np
import pytest
import torch

from tests import jpeg_cases as JC

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def fixture():
    return JC.load()


@functools.lru_cache(maxsize=None)
def decoder():
    from stp3_amd.datas import JpegDecoder
    return JpegDecoder(workers=2)


def differing(got, want):
    return int((got.cpu().numpy() != want).sum())


@pytest.mark.parametrize('name', JC.SUPPORTED)
def test_decoder_matches_pillow(name):
    g = fixture()
    got = decoder()(JC.streams(g, name), 'cuda')
    want = JC.expected(g, name)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    print(f'{name}: {differing(got, want)} of {want.size} bytes differ')
    assert differing(got, want) == 0, name


@pytest.mark.parametrize('name', JC.UNSUPPORTED)
def test_unsupported_streams_take_the_fallback(name):
    from stp3_amd.datas import JpegDecoder, JpegUnsupported
    g = fixture()
    got = decoder()(JC.streams(g, name), 'cuda')
    assert got.is_cuda and differing(got, JC.expected(g, name)) == 0, name
    with pytest.raises(JpegUnsupported, match='image 0'):
        JpegDecoder(fallback=False)(JC.streams(g, name), 'cuda')


def test_unsupported_streams_are_refused_without_the_fallback():
    from stp3_amd.datas import JpegDecoder, JpegUnsupported
    g = fixture()
    for name in JC.UNSUPPORTED:
        with pytest.raises(JpegUnsupported, match='image 1'):
            JpegDecoder(fallback=False)(JC.streams(g, 's420_16x16') + JC.streams(g, name), 'cuda')


def test_three_images_into_a_preallocated_output():
    g = fixture()
    out = torch.full((3, 32, 48, 3), 77, dtype=torch.uint8, device='cuda')
    got = decoder()(JC.streams(g, 's420_32x48_n3'), 'cuda', out=out)
    assert got is out and differing(out, JC.expected(g, 's420_32x48_n3')) == 0


def test_mixed_geometry_in_one_call():
    g = fixture()
    names = ('s420_40x40_q5', 's444_strips', 's420_40x40_opt', 'grey_13x9', 's420_40x40_q100')
    got = decoder()([JC.streams(g, n)[0] for n in names], 'cuda')
    assert isinstance(got, list) and [differing(a, JC.expected(g, n)[0]) for a, n in zip(got, names)] == [0] * 5


def test_captured_graph_replays_on_rewritten_buffers():
    """One stream, no parallel branches: the copy-free reconstruct on static tensors; the coefficient and table buffers are
    rewritten in place with another image set of the same geometry and the graph is replayed once."""
    g, dec = fixture(), decoder()
    first, second = (dec.entropy(JC.streams(g, k)) for k in ('s420_32x48_n3', 's420_32x48_n3_replay'))
    geometry = first.groups[0].geometry
    coef, quant = first.groups[0].coef.cuda(), first.groups[0].quant.cuda()
    out = torch.zeros(3, 32, 48, 3, dtype=torch.uint8, device='cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dec.reconstruct_device(geometry, coef, quant, out)                       # warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dec.reconstruct_device(geometry, coef, quant, out)
    graph.replay()
    torch.cuda.synchronize()
    assert differing(out, JC.expected(g, 's420_32x48_n3')) == 0
    coef.copy_(second.groups[0].coef)
    quant.copy_(second.groups[0].quant)
    graph.replay()
    torch.cuda.synchronize()
    assert differing(out, JC.expected(g, 's420_32x48_n3_replay')) == 0
    assert not np.array_equal(JC.expected(g, 's420_32x48_n3'), JC.expected(g, 's420_32x48_n3_replay'))


def test_decoder_feeds_the_image_preprocessor():
    """48 x 64 frames -> a 20 x 32 window: ImagePreprocessor on the decoder's output equals its torch statements on Pillow's bytes."""
    from stp3_amd.datas import ImagePreprocessor
    g = fixture()
    prep = ImagePreprocessor(resize_dims=(40, 30), crop=(4, 6, 36, 26), source_hw=(48, 64))
    images = decoder()(JC.streams(g, JC.CHAIN), 'cuda')
    got = prep(images)
    want = prep.reference(torch.from_numpy(JC.expected(g, JC.CHAIN)))
    assert tuple(got.shape) == (1, 3, 20, 32) and torch.equal(got.cpu(), want)
