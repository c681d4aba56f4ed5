"""The cases of the JPEG decoder's tests (tests/test_jpeg_cpu.py, tests/test_jpeg_gpu.py, tests/hipcpu/run_jpeg.py,
tests/test_jpeg_sanitize_cpu.py): the smallest shapes at which each mechanism of the decode can go wrong.

The SOURCE images are built here, deterministically; scripts/make_golden_jpeg.py encodes them with Pillow and stores the
byte streams and Pillow's decode in tests/golden/jpeg_cases.npz.  The tests read the stored streams: a different Pillow on
another machine cannot move them.  Every comparison of this feature is exact equality of every byte."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jpeg_cases.npz')
STRIP_420 = 32                                      # pixel rows a workgroup of the kernel owns at 4:2:0 (stp3_jpeg_strip_rows(2))

# name -> (height, width, what Pillow's save gets); 'images' > 1: several streams of one geometry for one launch.
# subsampling: Pillow's 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0.
CASES = {
    's444_8x8': dict(hw=(8, 8), save=dict(quality=90, subsampling=0)),                    # one block, no up-sampling
    's420_16x16': dict(hw=(16, 16), save=dict(quality=90, subsampling=2)),                # one MCU: every edge rule at once
    's420_23x37': dict(hw=(23, 37), save=dict(quality=85, subsampling=2)),                # partial MCUs, odd luma and chroma sizes
    's422_17x40': dict(hw=(17, 40), save=dict(quality=85, subsampling=1)),                # h2v1, (40 wide, 17 high)
    's422_40x17': dict(hw=(40, 17), save=dict(quality=85, subsampling=1)),                # h2v1, odd width
    's420_48x64_rst_row': dict(hw=(48, 64), save=dict(quality=80, subsampling=2, restart_marker_rows=1)),
    's420_48x64_rst_3': dict(hw=(48, 64), save=dict(quality=80, subsampling=2, restart_marker_blocks=3)),
    'grey_13x9': dict(hw=(13, 9), grey=True, save=dict(quality=90)),
    's420_40x40_q100': dict(hw=(40, 40), save=dict(quality=100, subsampling=2)),          # quantiser 1
    's420_40x40_q5': dict(hw=(40, 40), save=dict(quality=5, subsampling=2)),              # quantiser 255-class values, clamping
    's420_40x40_opt': dict(hw=(40, 40), save=dict(quality=75, subsampling=2, optimize=True)),   # custom Huffman tables
    's420_16x4': dict(hw=(16, 4), save=dict(quality=90, subsampling=2)),                  # chroma width 2: replication
    's422_9x3': dict(hw=(9, 3), save=dict(quality=90, subsampling=1)),                    # the same rule for h2v1
    's420_32x48_n3': dict(hw=(32, 48), images=3, save=[dict(quality=q, subsampling=2) for q in (50, 75, 95)]),
    's420_32x48_n3_replay': dict(hw=(32, 48), images=3, seed=50, save=[dict(quality=q, subsampling=2) for q in (95, 30, 60)]),
    's420_strips': dict(hw=(3 * STRIP_420 + 5, 64), save=dict(quality=90, subsampling=2)),   # the halo, a last partial strip
    's444_strips': dict(hw=(2 * 16 + 3, 24), save=dict(quality=90, subsampling=0)),
    # what the entropy decoder answers with STP3_EUNSUP: the fallback's ground
    'progressive': dict(hw=(24, 24), save=dict(quality=85, subsampling=2, progressive=True), unsupported=True),
    'cmyk': dict(hw=(16, 24), cmyk=True, save=dict(quality=85), unsupported=True),
    # (Pillow writes no 4:1:1: scripts/make_golden_jpeg.py assembles this stream itself from the tables of a Pillow stream)
    's411': dict(hw=(16, 40), handmade_411=True, save=dict(quality=85, subsampling=0), unsupported=True),
}
SUPPORTED = [k for k, c in CASES.items() if not c.get('unsupported')]
UNSUPPORTED = [k for k, c in CASES.items() if c.get('unsupported')]
TRUNCATE = ('s420_16x16', 'grey_13x9')              # every truncation of these (host sanitizer); the first one in the CPU tests
CHAIN = 's420_48x64_rst_row'                        # the decoder in front of ImagePreprocessor


def source(name, k=0):
    """The k-th source image of a case, (H, W, 3) uint8 (grey: (H, W); CMYK: (H, W, 4)): a smooth gradient, seeded noise and
    hard edges between saturated primaries, so that the range limit is reached in the IDCT and in the colour step."""
    c = CASES[name]
    h, w = c['hw']
    rng = np.random.RandomState(1000 + 17 * sorted(CASES).index(name) + c.get('seed', 0) + k)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(xx * 255) // max(w - 1, 1), (yy * 255) // max(h - 1, 1), ((xx + yy) * 255) // max(h + w - 2, 1)], axis=2)
    img = img + rng.randint(-40, 41, size=img.shape)
    primaries = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [255, 0, 255], [0, 255, 255], [255, 255, 255], [0, 0, 0]])
    for j in range(4):                                # rectangles of primaries: odd offsets, edges inside blocks
        y0, x0 = rng.randint(0, h), rng.randint(0, w)
        img[y0:y0 + 1 + h // 3, x0:x0 + 1 + w // 3] = primaries[(j + k + rng.randint(0, 8)) % 8]
    img = img.clip(0, 255).astype(np.uint8)
    if c.get('grey'):
        return img[:, :, 1].copy()
    if c.get('cmyk'):
        return np.concatenate([img, 255 - img[:, :, :1]], axis=2)
    return img


def crafted_grey(height, width, quant, dc_symbol, dc_bits, ac_symbol, ac_bits, blocks=None, sixteen_bit_quant=False):
    """A syntactically valid grey baseline stream whose every block is the same bits: a DC table with the single code '0'
    for `dc_symbol` followed by `dc_bits`, an AC table with the single code '0' for `ac_symbol` followed by `ac_bits`
    (give an end-of-block or a run to 63 so that the block ends).  `quant`: one value for all 64 entries.  What no encoder
    writes and a decoder of untrusted bytes must refuse without leaving its integer types."""
    n = blocks if blocks is not None else -(-height // 8) * -(-width // 8)
    seg = lambda m, body: bytes([0xFF, m]) + (len(body) + 2).to_bytes(2, 'big') + body
    dqt = bytes([0x10]) + quant.to_bytes(2, 'big') * 64 if sixteen_bit_quant else bytes([0x00]) + bytes([quant]) * 64
    table = lambda tc, sym: bytes([tc << 4]) + bytes([1] + [0] * 15) + bytes([sym])
    bits = ('0' + dc_bits + '0' + ac_bits) * n
    bits += '1' * (-len(bits) % 8)
    scan = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8)).replace(b'\xff', b'\xff\x00')
    return (b'\xff\xd8' + seg(0xDB, dqt) + seg(0xC0, bytes([8]) + height.to_bytes(2, 'big') + width.to_bytes(2, 'big') + bytes([1, 1, 0x11, 0])) +
            seg(0xC4, table(0, dc_symbol)) + seg(0xC4, table(1, ac_symbol)) + seg(0xDA, bytes([1, 1, 0x00, 0, 63, 0])) + scan + b'\xff\xd9')


def crafted_refused():
    """name -> a crafted stream the entropy decoder must answer with STP3_EINVAL."""
    return {
        # every block adds +32767 to the DC predictor: 66 049 blocks would walk it out of a 32-bit integer
        'dc_walks_away': crafted_grey(2056, 2048, 1, 15, '1' * 15, 0x00, ''),
        # ... and downwards
        'dc_walks_down': crafted_grey(512, 512, 1, 15, '0' * 15, 0x00, ''),
        # a DC inside 16 bits whose dequantised value is not: 300 * 255
        'dc_times_quant': crafted_grey(16, 16, 255, 9, '100101100', 0x00, ''),
        # an AC coefficient of 15 bits under a 16-bit quantiser: 32767 * 65535
        'ac_times_quant': crafted_grey(16, 16, 65535, 0, '', 0x0F, '1' * 15, sixteen_bit_quant=True),
    }


def load():
    """The stored fixture: '<case>/<k>/jpeg' (uint8 bytes of the stream) and '<case>/<k>/rgb' (Pillow's decode)."""
    return dict(np.load(GOLDEN))


def streams(fixture, name):
    return [fixture[f'{name}/{k}/jpeg'].tobytes() for k in range(CASES[name].get('images', 1))]


def expected(fixture, name):
    return np.stack([fixture[f'{name}/{k}/rgb'] for k in range(CASES[name].get('images', 1))])
