"""The cases of the device entropy decode of the JPEG decoder (tests/test_jpeg_huff_cpu.py, tests/test_jpeg_huff_gpu.py,
tests/test_jpeg_huff_host_cpu.py, tests/hipcpu/run_jpeg_huff.py): every SUPPORTED case of tests/jpeg_cases.py, plus the
smallest streams at which the mechanisms of the parallel decode can go wrong.

The source images are built here, deterministically; scripts/make_golden_jpeg_huff.py encodes them with Pillow and stores the
streams and the sha256 of Pillow's RGB decode in tests/golden/jpeg_huff_cases.npz.  Every comparison is exact equality."""
import hashlib
import os

import numpy as np

from tests import jpeg_cases as JC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jpeg_huff_cases.npz')
S, G = 128, 256                                      # STP3_JPEG_SUB_BYTES, STP3_JPEG_SUB_THREADS the fixture was built for

# name -> height, width, what Pillow's save gets (subsampling 0 = 4:4:4, 2 = 4:2:0), amplitude of the seeded noise
CASES = {
    'one_sub': dict(hw=(8, 8), noise=40, save=dict(quality=90, subsampling=0)),                 # one subsequence: nothing to synchronise
    'wg_sync': dict(hw=(96, 128), noise=40, save=dict(quality=95, subsampling=2)),             # synchronisation inside one workgroup
    'wg_sync_rst': dict(hw=(96, 128), noise=40, like='wg_sync', save=dict(quality=95, subsampling=2, restart_marker_rows=1)),
    'multi_wg': dict(hw=(320, 480), noise=60, save=dict(quality=95, subsampling=2)),           # more than three workgroups
    'stuff_edge': dict(hw=(96, 128), noise=40, search=True, save=dict(quality=95, subsampling=2)),   # stuffing at a subsequence edge
    'n3_mixed': dict(hw=(32, 48), noise=40, images=3, save=[dict(quality=35, subsampling=2), dict(quality=92, subsampling=2, optimize=True),
                                                             dict(quality=70, subsampling=2, restart_marker_blocks=2)]),
}
SWEEP = ('wg_sync', 'wg_sync_rst')                    # the corruption sweep of the emulator
CORRUPTIONS = 300


def source(name, k=0, seed=None):
    """The k-th source image of a case, (H, W, 3) uint8: gradients, seeded noise, rectangles of saturated primaries."""
    c = CASES[name]
    name = c.get('like', name)
    h, w = c['hw']
    rng = np.random.RandomState(7000 + 31 * sorted(CASES).index(name) + k if seed is None else seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(xx * 255) // max(w - 1, 1), (yy * 255) // max(h - 1, 1), ((xx + yy) * 255) // max(h + w - 2, 1)], axis=2)
    img = img + rng.randint(-c['noise'], c['noise'] + 1, size=img.shape)
    primaries = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [255, 0, 255], [0, 255, 255], [255, 255, 255], [0, 0, 0]])
    for j in range(4):
        y0, x0 = rng.randint(0, h), rng.randint(0, w)
        img[y0:y0 + 1 + h // 5, x0:x0 + 1 + w // 5] = primaries[(j + k + rng.randint(0, 8)) % 8]
    return img.clip(0, 255).astype(np.uint8)


def scan_offset(s):
    at = s.index(b'\xff\xda')
    return at + 2 + ((s[at + 2] << 8) | s[at + 3])


def walk(s, sub=S):
    """What stp3_jpeg_scan_prepare does with a regular stream, stated in Python: the entropy-coded bytes without byte
    stuffing, every restart interval padded with zeros to whole subsequences, and per segment (first subsequence, bits)."""
    pos, out, segments = scan_offset(s), bytearray(), []
    while True:
        start = len(out)
        while not (s[pos] == 0xFF and s[pos + 1] != 0x00):
            out.append(s[pos])
            pos += 2 if s[pos] == 0xFF else 1
        segments.append((start // sub, 8 * (len(out) - start)))
        out += bytes(-len(out) % sub if len(out) > start else sub)
        marker = s[pos + 1]
        pos += 2
        if marker == 0xD9:
            return bytes(out), segments
        assert marker == 0xD0 + (len(segments) - 1) % 8, hex(marker)


def stuffing_at_an_edge(s, sub=S):
    """(a stuffed FF 00 pair straddles a subsequence edge of the STUFFED scan, an FF is the last byte of a subsequence of the
    unstuffed one) for a stream without restart markers."""
    first, plain = scan_offset(s), walk(s, sub)[0]
    end = s.rindex(b'\xff\xd9')
    straddles = any(s[i] == 0xFF and s[i + 1] == 0x00 and (i - first) % sub == sub - 1 for i in range(first, end))
    return straddles, any(plain[i] == 0xFF for i in range(sub - 1, len(plain), sub))


def load():
    """The stored fixture, '<case>/<k>/jpeg' and '<case>/<k>/sha256', after checking that the cases still hit what they claim
    under the S and G of the library."""
    from stp3_amd import _lib
    g = dict(np.load(GOLDEN))
    s, wg = _lib.JPEG_SUB_BYTES, _lib.JPEG_SUB_THREADS
    nsub = lambda name: len(walk(streams(g, name)[0], s)[0]) // s
    assert nsub('one_sub') == 1
    assert 8 <= nsub('wg_sync') <= wg and len(walk(streams(g, 'wg_sync_rst')[0], s)[1]) == 96 // 16
    assert any(bits % (8 * s) for _, bits in walk(streams(g, 'wg_sync_rst')[0], s)[1])           # segments end mid-subsequence
    assert nsub('multi_wg') > 3 * wg, 'multi_wg must span more than three workgroups: grow the shape'
    assert stuffing_at_an_edge(streams(g, 'stuff_edge')[0], s) == (True, True), 'stuff_edge: search again for this S'
    return g


def streams(fixture, name):
    return [fixture[f'{name}/{k}/jpeg'].tobytes() for k in range(CASES[name].get('images', 1))]


def digest(rgb):
    return hashlib.sha256(np.ascontiguousarray(rgb, dtype=np.uint8).tobytes()).hexdigest()


def expected_digests(fixture, name):
    return [bytes(fixture[f'{name}/{k}/sha256']).hex() for k in range(CASES[name].get('images', 1))]


def all_cases():
    """(fixture key, case name) of every case the device decode is run on: the supported ones of tests/jpeg_cases.py first."""
    return [('jpeg', n) for n in JC.SUPPORTED] + [('huff', n) for n in CASES]
