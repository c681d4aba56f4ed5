"""GPU: the PNG decoder (stp3_amd.datas.PngDecoder; csrc/stp3_png.hip: stp3_png_unfilter) on the cases of tests/png_cases.py --
handmade streams against their source arrays, stored streams against the sha256 of Pillow's decode recorded in
tests/golden/png_cases.npz.  The streams behind the fallback are decoded by Pillow inside the call, which is the fallback --
without Pillow those tests FAIL, they do not skip.  Every comparison is exact equality of every byte."""
import functools

import numpy as np
import pytest
import torch

from tests import png_cases as PC

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def fixture():
    return PC.load()


@functools.lru_cache(maxsize=None)
def decoder():
    from stp3_amd.datas import PngDecoder
    return PngDecoder(workers=2)


@pytest.mark.parametrize('name', PC.SUPPORTED)
def test_decoder_matches(name):
    g = fixture()
    got = decoder()(PC.streams(g, name), 'cuda')
    assert got.is_cuda and got.dtype == torch.uint8
    want = PC.expected(g, name)
    if want is not None:
        assert tuple(got.shape) == want.shape
        differ = int((got.cpu().numpy() != want).sum())
        print(f'{name}: {differ} of {want.size} bytes differ')
        assert differ == 0, name
    assert PC.matches(g, name, got.cpu().numpy()), name


@pytest.mark.parametrize('name', PC.UNSUPPORTED)
def test_unsupported_streams_take_the_fallback(name):
    from stp3_amd.datas import PngDecoder, PngUnsupported
    g = fixture()
    got = decoder()(PC.streams(g, name), 'cuda')
    assert got.is_cuda and PC.matches(g, name, got.cpu().numpy()), name
    with pytest.raises(PngUnsupported, match='image 1'):
        PngDecoder(fallback=False)(PC.streams(g, 'only_type_4') + PC.streams(g, name), 'cuda')


def test_sixteen_bit_grey_is_refused_not_cut_to_eight_bits():
    from stp3_amd.datas import PngDecoder, PngUnsupported
    g = fixture()
    for dec in (decoder(), PngDecoder(fallback=False)):
        with pytest.raises(PngUnsupported, match='image 1: 16-bit samples'):
            dec(PC.streams(g, 'only_type_4') + [PC.unsupported_stream('grey_16bit')], 'cuda')


def test_mixed_geometry_in_one_call():
    g = fixture()
    names = ('only_type_4', 'grey_65x257', 'only_type_3', 'rgba_70x33', 'rgb_16bit', 'only_type_1', 'grey_1bit')
    got = decoder()([PC.streams(g, n)[0] for n in names], 'cuda')
    assert isinstance(got, list) and all(a.dtype == torch.uint8 for a in got) and all(PC.matches(g, n, a.cpu().numpy()[None]) for a, n in zip(got, names))


def test_captured_graph_replays_on_rewritten_buffers():
    """One stream, no parallel branches: the copy-free unfilter on static tensors; the scanline buffer is rewritten in place with
    another image set of the same geometry and the graph is replayed once."""
    g, dec = fixture(), decoder()
    first, second = (dec.inflate(PC.streams(g, k)) for k in ('three_images', 'three_images_replay'))
    geometry = first.groups[0].geometry
    rows = first.groups[0].rows.cuda()
    out = torch.zeros(3, 20, 24, 3, dtype=torch.uint8, device='cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dec.unfilter_device(geometry, rows, out)                                  # warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dec.unfilter_device(geometry, rows, out)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), PC.expected(g, 'three_images'))
    rows.copy_(second.groups[0].rows)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), PC.expected(g, 'three_images_replay'))
    assert not np.array_equal(PC.expected(g, 'three_images'), PC.expected(g, 'three_images_replay'))


@pytest.mark.parametrize('name', ('band_130x33', 'pass_515x5', 'wide_2x16384', 'grey_65x257', 'rgba_70x33', 'three_images', 'extreme_9x1_c2'))
def test_a_guard_ring_around_the_output_stays_untouched(name):
    g, dec = fixture(), decoder()
    grp = dec.inflate(PC.streams(g, name)).groups[0]
    want = PC.expected(g, name)
    ring = 256
    buf = torch.full((want.size + 2 * ring,), 77, dtype=torch.uint8, device='cuda')
    out = buf[ring:ring + want.size].view(want.shape)
    dec.unfilter_device(grp.geometry, grp.rows.cuda(), out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want), name
    assert bool((buf[:ring] == 77).all()) and bool((buf[-ring:] == 77).all()), name


def test_load_carla_sample_from_bytes_on_the_gpu():
    """The sample of tests/png_cases.py from its files' bytes on the GPU == assemble_carla_sample on host-decoded arrays
    uploaded as they are: every key, bit for bit."""
    from stp3_amd import carla
    files, arrays, m = PC.carla_files()
    dec = carla.CarlaDecoder(crop=256, bev_crop=200)
    seeded = lambda: torch.Generator(device='cuda').manual_seed(3)
    got = carla.load_carla_sample(dec, decoder(), **files, **m, generator=seeded(), device='cuda')
    want = carla.assemble_carla_sample(dec, *(torch.from_numpy(a).cuda() for a in arrays), **m, generator=seeded())
    assert got['image'].is_cuda and tuple(got['image'].shape) == (2, 4, 3, 256, 256)
    assert PC.sample_difference(got, want) == []
